// thip_encode_entry.h -- what the direct entries of thip_encode.hip (thip_enc_*_stage, thip_enc_pack_tokens; theora_hip.h) share,
// host code: the frame rule, the picture-and-planes rule, the builders of the kernels' EncPlanes and EncRef, and three small items (an
// alignment test, a table range test, a device allocation that frees itself).  An entry reads: validate with these, build with these,
// allocate the scratch it alone needs, launch, synchronise.  Nothing here touches a device but DeviceBuf.
//
// The picture region of a plane (spec 4.4) is pic_span's: th_encode_alloc and enc_queue_frame take theirs from it too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/theora_hip.h"
#include "thip_bitstream.h"
#include "thip_encode_inter.h"

namespace thip {

inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }   // a: a power of two

// every one of a table's n entries lies in [lo, hi]
template <class T>
bool table_within(const T *t, size_t n, int lo, int hi) {
  for (size_t k = 0; k < n; k++)
    if (t[k] < lo || t[k] > hi) return false;
  return true;
}

// device memory for the lifetime of the object; one that never allocated frees nothing
struct DeviceBuf {
  uint8_t *p = nullptr;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf &) = delete;
  DeviceBuf &operator=(const DeviceBuf &) = delete;
  ~DeviceBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc((void **)&p, bytes); }
};

// ---- the frame rule: a coded frame of whole macro blocks below 1 << 20 a side, a pixel format of the specification, and no more than
// max_frags blocks in its three planes
constexpr int64_t kEntryMaxFrags = (int64_t)1 << 24;
struct EntryFrame {
  int width, height, hdec, vdec;
  int64_t nluma, nfrags;   // blocks of the luma plane, of the three planes
};
inline int check_frame(EntryFrame &f, int width, int height, int pixel_fmt, int64_t max_frags = kEntryMaxFrags) {
  if (width <= 0 || height <= 0 || (width & 15) || (height & 15) || width >= (1 << 20) || height >= (1 << 20)) return THIP_EINVAL;
  if (pixel_fmt < 0 || pixel_fmt >= TH_PF_NFORMATS || pixel_fmt == TH_PF_RSVD) return THIP_EINVAL;
  f.width = width;
  f.height = height;
  f.hdec = !(pixel_fmt & 1);
  f.vdec = !(pixel_fmt & 2);
  f.nluma = (int64_t)(width >> 3) * (height >> 3);
  f.nfrags = f.nluma + 2 * (f.nluma >> (f.hdec + f.vdec));
  return f.nfrags > max_frags ? THIP_EINVAL : THIP_OK;
}

// ---- the picture-and-planes rule
struct PicRect {   // the picture in its coded frame, display coordinates (row 0 at the top), as th_info has it
  int x, y, w, h;
};
template <class Req>
PicRect pic_rect(const Req &q) { return PicRect{q.pic_x, q.pic_y, q.pic_width, q.pic_height}; }

// the samples [x, x + w) of the luma plane in a plane decimated by `dec` (spec 4.4): the first, and how many
struct PicSpan {
  int x0, n;
};
inline PicSpan pic_span(int x, int w, int dec) { return PicSpan{x >> dec, ((x + w + dec) >> dec) - (x >> dec)}; }

inline bool pic_outside(const PicRect &r, int frame_width, int frame_height) {
  return r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 || r.w > frame_width || r.h > frame_height || r.x > frame_width - r.w ||
         r.y > frame_height - r.h;
}

// a request's planes: the source's with src_pitch, the references' with ref_pitch.  What the request has no field for stays NULL
struct EntryPlanes {
  const uint8_t *const *src;
  const int64_t *src_pitch;
  const uint8_t *const *prev, *const *gold;
  const int64_t *ref_pitch;
};
enum class Gold { ignored, required, forbidden };

// THIP_EFAULT where a plane the call reads is NULL -- the source's always, PREV's when it reads references (refs), GOLD's when
// required --, THIP_EINVAL where a GOLD plane is given and forbidden
inline int check_plane_pointers(const EntryPlanes &pl, bool refs, Gold gold) {
  int ngold = 0;
  for (int p = 0; p < 3; p++) {
    if (!pl.src[p] || (refs && !pl.prev[p])) return THIP_EFAULT;
    ngold += pl.gold && pl.gold[p];
  }
  if (gold == Gold::required && ngold < 3) return THIP_EFAULT;
  if (gold == Gold::forbidden && ngold) return THIP_EINVAL;
  return THIP_OK;
}

// a source row shorter than the picture's part of the plane; with refs, a reference row shorter than the frame's or beyond 31 bits
inline bool pitches_outside(const EntryFrame &f, const PicRect &r, const EntryPlanes &pl, bool refs) {
  for (int p = 0; p < 3; p++) {
    const int hd = p ? f.hdec : 0;
    if (pl.src_pitch[p] < pic_span(r.x, r.w, hd).n) return true;
    if (refs && (pl.ref_pitch[p] < (f.width >> hd) || pl.ref_pitch[p] > 0x7FFFFFFF)) return true;
  }
  return false;
}

// the three in the order every entry keeps: the rectangle (THIP_EINVAL), the pointers, the pitches (THIP_EINVAL)
inline int check_picture_planes(const EntryFrame &f, const PicRect &r, const EntryPlanes &pl, bool refs, Gold gold) {
  if (pic_outside(r, f.width, f.height)) return THIP_EINVAL;
  if (const int rc = check_plane_pointers(pl, refs, gold)) return rc;
  return pitches_outside(f, r, pl, refs) ? THIP_EINVAL : THIP_OK;
}

// ---- the builders
// the kernels' view of a frame's blocks and of the picture in it, read through src / stride (the picture's top-left pixel of each plane;
// NULL: no kernel of the call reads pixels)
inline EncPlanes enc_planes(const FrameGeometry &geo, const PicRect &r, const uint8_t *const src[3], const int64_t stride[3]) {
  EncPlanes g = {};
  for (int p = 0; p < 3; p++) {
    const PicSpan sx = pic_span(r.x, r.w, p ? geo.hdec : 0), sy = pic_span(r.y, r.h, p ? geo.vdec : 0);
    if (src) {
      g.src[p] = src[p];
      g.stride[p] = stride[p];
    }
    g.px0[p] = sx.x0;
    g.py0[p] = sy.x0;
    g.pw[p] = sx.n;
    g.ph[p] = sy.n;
    g.nh[p] = geo.nh[p];
    g.nv[p] = geo.nv[p];
    g.froff[p] = geo.fro[p];
  }
  return g;
}

// a reference of the frame's size in the caller's planes (NULL: the call reads none, and only the decimation is set)
inline EncRef enc_ref(const FrameGeometry &geo, const uint8_t *const plane[3], const int64_t pitch[3]) {
  EncRef R = {};
  for (int p = 0; p < 3 && plane; p++) {
    R.plane[p] = plane[p];
    R.stride[p] = (int)pitch[p];
    R.w[p] = geo.nh[p] * 8;
    R.h[p] = geo.nv[p] * 8;
  }
  R.hdec = geo.hdec;
  R.vdec = geo.vdec;
  return R;
}

}  // namespace thip
