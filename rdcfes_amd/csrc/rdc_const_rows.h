// rdc_const_rows.h — when an element-visit launch of the PIHNA assembly (k_tet4_ev / k_tet4_evq, rdc_tet4_ev.hip) may leave the
// rows of the a equation (cytokine: row 4 of every node) as an earlier launch wrote them.
//
//   A[4][*] = (0, -T sec_c, -T sec_h, T upt a, 1 + T (upt v + dec))   ->   o[20..24] of ev::pihna_expand (rdc_tet4_ev.h)
//
// With uptake/a/from/v = 0 (the shipped value) these entries are the mass moment E1 of the mesh times Tsec_c, Tsec_h and 1 + Tdec:
// nothing of the unknowns, which are all that changes from one time step to the next.  They are a fifth of the CSR values, the
// last 5 len doubles of every node's contiguous segment of 25 len.  A launch that finds them in memory writes four rows (NROW = 4).
//
// The decision is made here and the launch code obeys it (assemble_rd, rdc_capi.hip): one record per context, "the a rows in
// memory are those of key K, over the rows of part 1 / part 2".  Host only (no HIP), no allocation: the CPU suite compiles it
// with g++ (tests/host_const_rows_main.cpp).
#ifndef RDC_CONST_ROWS_H
#define RDC_CONST_ROWS_H
#include <stdint.h>

namespace rdc {

// the values that enter o[20..24], as PihnaK holds them (Pihna::derive), and whether the state-dependent terms are absent
struct ConstRowsKey {
  double Tsec_c = 0.0, Tsec_h = 0.0, Tdec = 0.0;
  bool upt0 = false;   // Tupt == 0
  bool same(const ConstRowsKey& o) const { return Tsec_c == o.Tsec_c && Tsec_h == o.Tsec_h && Tdec == o.Tdec && upt0 == o.upt0; }   // a NaN never matches
};
template <class K>
ConstRowsKey const_rows_key(const K& k) { return ConstRowsKey{k.Tsec_c, k.Tsec_h, k.Tdec, k.Tupt == 0.0}; }

// option "const_rows" (rdc_set_option): 0 = every launch writes every row, 1 = as decided below (default), 2 = as 1, and the caller
// promises not to write the value or coordinate arrays through the pointers it was given.  Kept beside the two tables of
// rdc_options.h: it is a contract, not a setting, and those tables' keys are fixed lists the CPU suite holds them to
constexpr const char* CONST_ROWS_REFUSED = "const_rows must be 0 (always write every row), 1 or 2 (1, and the caller does not write through device pointers)";
inline bool const_rows_mode_ok(const int v) { return v >= 0 && v <= 2; }

struct ConstRows {
  int mode = 1;                     // option "const_rows"; a setting of the context: nothing below resets it
  // ---- the record: a completed enqueue of a five-row launch on the element-visit path sets it for its part
  bool valid[2] = {false, false};   // the rows that part 1 / part 2 own hold the a rows of `key` (a whole assembly: both)
  ConstRowsKey key;
  int64_t interior = -1;            // "interior_nodes" at that launch: the two-part split the two flags refer to
  // ---- mutable device pointers in the caller's hands: it may write through them at any later time
  bool values_out = false;          // rdc_csr_values_device_ptr gave out the value array: no skipping until the next rdc_mesh_upload
  bool coords_out = false;          // rdc_mesh_coords_device_ptr gave out the coordinates: none for the life of the context
  // ---- launches recorded into a graph: a replay writes the five rows of ITS key at a time the host does not see, so from the
  // capture on only that key may be skipped (a second captured key: none), until the next rdc_mesh_upload ends the graph's validity
  bool captured = false, captured_mixed = false;
  ConstRowsKey captured_key;

  void clear() { valid[0] = valid[1] = false; }
  // rdc_mesh_upload: new value array, new lists; graphs and value pointers of the old mesh are void
  void mesh_upload() { clear(); values_out = false; captured = captured_mixed = false; }
  // rdc_mesh_update_coords: E1 changes
  void coords_update() { clear(); }
  // an assembly of the context through another kernel path or another model, or with a timing-only build of the kernels
  void other_assembly() { clear(); }
  void values_pointer() { values_out = true; }
  void coords_pointer() { coords_out = true; }

  // Rows (5 or 4) a launch on the element-visit path writes.  mode: option "const_rows" (0 = always five, 1 = as below, 2 = as 1,
  // and the caller promises not to write through the pointers it was given); part: 0 = whole, 1, 2; interior: "interior_nodes" of
  // the call; capturing: the stream records into a graph -- such a launch writes everything, whatever the host knows now
  int rows(const int mode, const ConstRowsKey& k, const int part, const int64_t interior_now, const bool capturing) {
    if (interior_now != interior) { clear(); interior = interior_now; }   // another split (or the first call): the flags mean nothing
    if (mode == 0 || capturing || !k.upt0) return 5;
    if (mode != 2 && (values_out || coords_out)) return 5;
    if (captured && (captured_mixed || !k.same(captured_key))) return 5;
    if (!k.same(key)) return 5;
    const bool have = part == 0 ? (valid[0] && valid[1]) : (part == 1 ? valid[0] : valid[1]);
    return have ? 4 : 5;
  }

  // What a launch that rows() decided leaves behind.  ok: the enqueue succeeded
  void launched(const int nrow, const ConstRowsKey& k, const int part, const bool capturing, const bool ok) {
    if (!ok) { clear(); return; }
    if (capturing) {   // the record stays as it is
      if (captured && !k.same(captured_key)) captured_mixed = true;
      if (!captured) { captured = true; captured_key = k; }
      return;
    }
    if (nrow != 5) return;   // four rows: nothing new in memory
    if (!k.same(key)) { clear(); key = k; }
    if (part == 0) valid[0] = valid[1] = true;
    else valid[part == 1 ? 0 : 1] = true;
  }
};

}  // namespace rdc
#endif
