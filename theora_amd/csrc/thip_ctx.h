// thip_ctx.h -- the leading part that th_dec_ctx (thip_frontend.cpp) and th_enc_ctx (thip_encode.hip) share, so that
// th_granule_frame and th_granule_time accept either kind of context, as libtheora's do.
#pragma once
#include "../../include/theoradec_hip.h"

struct thip_ctx_head {
  th_info info;
  int granpos_bias;   // 1 for bitstream 3.2.1 and later: frames are counted from 1 (state.c:740-745)
};

// the backend state of a th_dec_ctx (thip_frontend.cpp): the encoder's reconstruction is a decoder of its own packets
struct thip_state;
thip_state *thip_dec_backend(th_dec_ctx *d);
