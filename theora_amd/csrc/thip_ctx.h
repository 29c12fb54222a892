// thip_ctx.h -- what the host sources share without HIP: the leading part of th_dec_ctx (thip_frontend.cpp) and th_enc_ctx
// (thip_encode.hip), so that th_granule_frame and th_granule_time accept either kind of context, as libtheora's do; a spinning
// thread's pause and the monotonic clock.
#pragma once
#include <time.h>

#include <thread>

#include "../../include/theoradec_hip.h"

struct thip_ctx_head {
  th_info info;
  int granpos_bias;   // 1 for bitstream 3.2.1 and later: frames are counted from 1 (state.c:740-745)
};

// the backend state of a th_dec_ctx (thip_frontend.cpp): the encoder's reconstruction is a decoder of its own packets
struct thip_state;
thip_state *thip_dec_backend(th_dec_ctx *d);

// a spinning thread's pause: the x86 hint where there is one (the unguarded builtin kept other hosts from compiling)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::this_thread::yield();
#endif
}
static inline double thip_now() {   // seconds on the monotonic clock
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
