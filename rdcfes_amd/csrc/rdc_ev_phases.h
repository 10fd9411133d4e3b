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

// ---- copy-out: one contiguous CSR segment per node, from the LDS image to memory with 16-byte non-temporal stores ----------------
typedef double v2d_t __attribute__((ext_vector_type(2)));
typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));

// a row has at most MAX_ROW_BLOCKS node blocks (the 4-bit slots of vslot_get, the slice's NBP / MAXN blocks per node), so a lane
// reads at most seg_reads(nv2) pieces of 16 bytes of a segment of nv2 values per block: 4 for 25 values, 2 for 9
constexpr int MAX_ROW_BLOCKS = HostPrepEv::NBP / HostPrepEv::MAXN;
static_assert(MAX_ROW_BLOCKS == 16, "vslot_get / block_slot: four bits per column slot");
constexpr int seg_reads(const int nv2) { return (nv2 * MAX_ROW_BLOCKS / 2 + 63) / 64; }

// The compiler may not split a batch of LDS reads: the empty statement needs every value of the batch in its register, so the
// reads in front of it are all issued before the one wait it causes (left to itself it sinks each read to its use: a round trip each)
__device__ __forceinline__ void lds_batch() { __builtin_amdgcn_sched_barrier(0); }
template <class T> __device__ __forceinline__ void lds_land(T& a) { asm volatile("" : "+v"(a)); }
template <class T> __device__ __forceinline__ void lds_land(T& a, T& b) { asm volatile("" : "+v"(a), "+v"(b)); }
template <class T> __device__ __forceinline__ void lds_land(T& a, T& b, T& c, T& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
template <int I = 0, class T, int N> __device__ __forceinline__ void lds_land(T (&r)[N]) {
  if constexpr (N - I >= 4) { lds_land(r[I], r[I + 1], r[I + 2], r[I + 3]); lds_land<I + 4>(r); }
  else if constexpr (N - I >= 2) { lds_land(r[I], r[I + 1]); lds_land<I + 2>(r); }
  else if constexpr (N - I == 1) lds_land(r[I]);
}

// the table entries of N nodes of a wave -- nodes first, first + 4, ... (uniform; first + 4 (N - 1) < MAXN) -- in scalar registers:
// read together (wave_nodes_read; `snode`: aligned to 16 bytes) and waited for once (wave_nodes_land, behind whatever else the
// caller reads with them)
template <int N>
__device__ __forceinline__ void wave_nodes_read(const HostPrepEv::Node* snode, const int first, v4u_t (&raw)[N]) {
  static_assert(sizeof(HostPrepEv::Node) == 16, "one 16-byte LDS read per entry");
#pragma unroll
  for (int q = 0; q < N; q++) raw[q] = reinterpret_cast<const v4u_t*>(snode)[first + 4 * q];
}
template <int N>
__device__ __forceinline__ void wave_nodes_land(v4u_t (&raw)[N], HostPrepEv::Node (&nd)[N]) {
  lds_batch();
  lds_land(raw);
#pragma unroll
  for (int q = 0; q < N; q++) {
    const uint32_t lb = __builtin_amdgcn_readfirstlane(raw[q].y);
    nd[q].bptr = __builtin_amdgcn_readfirstlane(raw[q].x);
    nd[q].len = (uint16_t)(lb & 0xFFFFu); nd[q].blk0 = (uint16_t)(lb >> 16);
    nd[q].obase = __builtin_amdgcn_readfirstlane(raw[q].z);
    nd[q].node = __builtin_amdgcn_readfirstlane(raw[q].w);
  }
}
template <int N>
__device__ __forceinline__ void wave_nodes(const HostPrepEv::Node* snode, const int first, HostPrepEv::Node (&nd)[N]) {
  v4u_t raw[N];
  wave_nodes_read(snode, first, raw);
  wave_nodes_land(raw, nd);
}

// one wave copies the CSR segments of NS nodes (NV2 = nvar^2 values per block; entries uniform, as wave_nodes gives them; on[s]:
// uniform, false = no such node; NS = 2 wherever the registers allow it) in one go: every LDS read of the segments -- 16 bytes per lane and read, the odd head and tail
// doubles with them -- is issued into registers of its own and waited for once, then the stores leave.  `image` holds the image
// from offset `base` (even) on; out[x] <-> img[x]: the image has the 16-byte phase of the segment in memory.  A lane past the end of
// its segment reads the segment's first piece (inside the image whatever the workgroup's LDS size) and stores nothing.
// NVW < NV2 (a multiple of nvar: whole equation rows): only the first NVW * len values of every segment leave -- the trailing rows
// keep what memory holds (rdc_const_rows.h); the image and the segment's place in memory are those of NV2 values per block.
template <int NV2, int NS, int NVW = NV2>
__device__ __forceinline__ void store_segments(const double* image, double* val, const HostPrepEv::Node (&nd)[NS], const bool (&on)[NS],
                                               const int lane, const uint32_t base = 0) {
  static_assert(NVW > 0 && NVW <= NV2, "the leading NVW of a block's NV2 values");
  constexpr int NR = seg_reads(NVW);
  v2d_t r[NS][NR];
  double ends[NS][2];   // the odd head and tail doubles
  const double* img[NS];
  int cnt[NS], sh[NS], npair[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) {
    img[s] = image + (on[s] ? nd[s].obase - base : 0u);
    cnt[s] = on[s] ? NVW * (int)nd[s].len : 0;
    sh[s] = on[s] ? seg_phase(nd[s].obase) : 0;
    npair[s] = (cnt[s] - sh[s]) >> 1;
    const v2d_t* src = reinterpret_cast<const v2d_t*>(img[s] + sh[s]);
#pragma unroll
    for (int i = 0; i < NR; i++) {
      const int x = lane + 64 * i;
      r[s][i] = src[x < npair[s] ? x : 0];
    }
    ends[s][0] = img[s][0];
    ends[s][1] = img[s][cnt[s] > 0 ? cnt[s] - 1 : 0];
  }
  lds_batch();
#pragma unroll
  for (int s = 0; s < NS; s++) { lds_land(r[s]); lds_land(ends[s]); }
#pragma unroll
  for (int s = 0; s < NS; s++) {
    double* out = val + (size_t)NV2 * nd[s].bptr;
    v2d_t* dstg = reinterpret_cast<v2d_t*>(out + sh[s]);
#pragma unroll
    for (int i = 0; i < NR; i++) {
      const int x = lane + 64 * i;
      if (x < npair[s]) __builtin_nontemporal_store(r[s][i], dstg + x);
    }
    if (sh[s] && lane == 0) __builtin_nontemporal_store(ends[s][0], out);
    if (((cnt[s] - sh[s]) & 1) && lane == 1) __builtin_nontemporal_store(ends[s][1], out + cnt[s] - 1);
  }
}

}  // namespace evl
}  // namespace rdc
#endif
