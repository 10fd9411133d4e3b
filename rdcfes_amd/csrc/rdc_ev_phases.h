// rdc_ev_phases.h — the device-only phases that k_tet4_ev, k_tet4_evq (rdc_tet4_ev.hip) and k_tet4_evc (rdc_tet4_evc.hip) share.
// The format of the lists they decode is evl:: (rdc_prep.h), which the host builder and the CPU replays compile too.
#ifndef RDC_EV_PHASES_H
#define RDC_EV_PHASES_H
#include "rdc_prep.h"

namespace rdc {
namespace evl {

// Zero BYTES of LDS at `lds`, a quarter per wave (`wave`: uniform, 0..3).  A store moves its address and data registers to the
// LDS at 2 cycles per source dword and wave instruction (MI355X_MICROARCH.md, LDS): ds_write_addtid_b32 has no address
// register (address = M0 + offset + 4 * lane), so zeroing a 32 KB slice costs 2 cycles per 256 bytes instead of 13 per
// 1024 with 16-byte stores.  M0 is restored (the LDS-DMA of the callers sets it too).
template <int BYTES>
__device__ __forceinline__ void zero_slice(const double* lds, const int wave) {
  static_assert(BYTES % (4 * 1024) == 0, "zeroing: 4 waves x groups of four addtid stores of 256 bytes");
  constexpr int PER_WAVE = BYTES / 4;
  const uint32_t zbase = (uint32_t)(uintptr_t)lds + (uint32_t)wave * (uint32_t)PER_WAVE;
  const uint32_t zero = 0u;
  uint32_t m0_saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0" : "=&s"(m0_saved) : "s"(zbase) : "memory");
#pragma unroll
  for (int o = 0; o < PER_WAVE; o += 1024)
    asm volatile("ds_write_addtid_b32 %0 offset:%1\n\tds_write_addtid_b32 %0 offset:%1+256\n\tds_write_addtid_b32 %0 offset:%1+512\n\tds_write_addtid_b32 %0 offset:%1+768"
                 :: "v"(zero), "n"(o) : "memory");
  asm volatile("s_mov_b32 m0, %0" :: "s"(m0_saved) : "memory");
}

// node records in LDS: pieces of 16 bytes, [piece][list position] (an LDS-DMA of one wave lands one piece of 64 consecutive positions)
__device__ __forceinline__ double* rec_at(double* recs, const int nls, const int p, const int pos) { return recs + (p * nls + pos) * 2; }
__device__ __forceinline__ double2 rec_piece(const double* recs, const int nls, const int p, const int pos) {
  return reinterpret_cast<const double2*>(recs)[p * nls + pos];
}

// where a visit adds: sink.pr[i] = rhs entry 0 of row i's node, sink.p[i][j] = entry / moment 0 of block (row i, column j); rows
// i >= r are not emitted and aim at node 0.  li: the visit's list positions (owned first: position == cluster index)
template <class Sink>
__device__ __forceinline__ void aim(Sink& sink, double* lds, double* R, const int (&li)[4], const int r, const uint2 sl) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int a = (i < r) ? li[i] : 0;
    sink.pr[i] = R + a;
#pragma unroll
    for (int j = 0; j < 4; j++) sink.p[i][j] = lds + block(a, vslot_get(sl.x, sl.y, i, j));
  }
}

// one wave copies the CSR segment of node nd (nv2 = nvar^2 values per block) from the LDS image to memory with 16-byte non-temporal
// stores; `image` holds the image from offset `base` (even) on; out[x] <-> img[x]: the image has the 16-byte phase of the segment in memory
__device__ __forceinline__ void store_segment(const double* image, double* val, const int nv2, const HostPrepEv::Node nd, const int lane,
                                              const uint32_t base = 0) {
  const double* img = image + (nd.obase - base);
  double* out = val + (size_t)nv2 * nd.bptr;
  const int cnt = nv2 * (int)nd.len, sh = seg_phase(nd.obase);
  typedef double v2d_t __attribute__((ext_vector_type(2)));
  const int npair = (cnt - sh) >> 1;
  const v2d_t* src = reinterpret_cast<const v2d_t*>(img + sh);
  v2d_t* dstg = reinterpret_cast<v2d_t*>(out + sh);
  for (int x = lane; x < npair; x += 64) __builtin_nontemporal_store(src[x], dstg + x);
  if (sh && lane == 0) __builtin_nontemporal_store(img[0], out);
  if (((cnt - sh) & 1) && lane == 1) __builtin_nontemporal_store(img[cnt - 1], out + cnt - 1);
}

}  // namespace evl
}  // namespace rdc
#endif
