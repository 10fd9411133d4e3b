// rdc_path.h — which kernel a reaction-diffusion assembly call (rdc_assemble_pihna / ripf / hcc / adpm / proteas and their _part
// forms) runs: the one place that decides it ("Which kernel runs").  assemble_rd fills Facts, builds the lists that
// path_builds asks for, and hands the Plan of path_decide to the launchers, which switch on it; rdc_part1_nodes asks the same
// function for its prediction.  Host only (no HIP) and pure: no allocation, no context, lists are "present or not".  The CPU suite
// compiles it with g++ (tests/host_shim.cpp, tests/test_host_path.py).
#ifndef RDC_PATH_H
#define RDC_PATH_H
#include "rdc_options.h"

namespace rdc {

// the kernel family a call ends in
enum class Path {
  TET4_CL,            // k_tet4_cl (rdc_tet4_cluster_mode)
  TET4_EV,            // k_tet4_ev / k_tet4_evq: PIHNA moments per element visit (Plan::ev_general: all 22 moments)
  TET4_EVC,           // k_tet4_evc: element visits in coefficient form
  TET4_RG5,           // the pair kernels, newest first
  TET4_RG3,
  TET4_RG2,
  TET4_ROWGATHER,     // k_tet4_rowgather
  TET4_COLOURED,      // k_tet4_coloured
  HEX8_CL,            // k_hex8_cl, three unknowns
  HEX8_CL_ROWS,       // k_hex8_cl one equation row at a time, five unknowns
  GENERIC_ROWGATHER,  // k_rowgather, plain or node-staged
  GENERIC_COLOURED    // k_coloured
};

// the model instantiation that runs
enum class Inst {
  FULL,     // the model of the call
  SPARSE,   // its parameter-sparsity variant: PihnaNoCellTransport, RipfReduced, HccMassOnly, AdpmDecayOnly
  MOMENTS   // PihnaNoCellTransportMoments: the sparse PIHNA rows in moment form
};

// what part 1 and part 2 of a two-part step launch
enum class TwoPart {
  WHOLE,         // "part" = 0
  EV_SPLIT,      // element-visit clusters: the interior ones / the rest
  CL_SPLIT,      // cluster lists (HEX8 kernels, k_tet4_cl): the leading interior clusters / the rest
  PAIR_SPLIT,    // k_tet4_rg5 workgroups: the leading interior ones / the rest
  ALL_IN_PART2   // the path launches no sub-range: nothing in part 1, everything in part 2
};

// a model, as far as the decision reads it (filled from M where assemble_rd is instantiated: describe<M>(), rdc_models.h)
struct PathModel {
  int nv;                 // unknowns per node
  bool per_elem;          // per-element inputs (M::NELEM > 0)
  bool aux_local;         // aux values read at one local node only (M::AUX_LOCAL_NODE >= 0)
  bool pihna;
  bool evc_eligible;      // its FULL instantiation has k_tet4_evc (EvcEligible)
  bool cl_mode1;          // takes k_tet4_cl in mode 1 of rdc_tet4_cluster_mode (Tet4ClWanted)
  bool sparse_tet4_only;  // the SPARSE instantiation exists for the TET4 kernels only (PIHNA, RIPF)
  bool sparse_per_elem;   // the SPARSE instantiation still reads the per-element inputs
};

struct Facts {
  int nen = 4;
  int strategy = RDC_SCATTER_ROWGATHER;   // resolved: never AUTO
  int variant = RDC_VARIANT_AUTO;
  Options opt;                            // "part" and "interior_nodes" included
  int tet4_cl_mode = 0;
  bool pattern = false;        // the model's sparsity pattern applies to the parameter values of the call
  bool stamps = false;         // diagnostic stamps are armed (rdc_debug_stamps)
  // the lists of the mesh
  bool rowgather_ok = false;   // generic row gather / k_tet4_rowgather: there are workgroups to launch
  bool rg2_ok = false;         // TET4 pair lists ...
  int rg2_block = 256;         // ... their workgroup size
  bool pair_aux = false, nlist = false;   // ... with the aux table (rg3, rg5) and the node lists (rg5)
  bool pair_eid = false;       // ... and the host has the pair -> element list, uploaded for the models that read it
  bool ev_ok = false;          // element-visit lists
  bool ev_tried = false;       // ... have been built or found impossible
  bool cl_ready = false;       // cluster lists exist for the current options (after the builds of path_builds: whichever it asked for)
  bool cl_fits = false;        // ... and the image of k_tet4_cl fits the device's LDS
};

struct Builds { bool ev = false, tet4_cl = false, hex8_cl = false, pair_eid = false; };

struct Plan {
  Path path = Path::GENERIC_COLOURED;
  Inst inst = Inst::FULL;
  TwoPart two_part = TwoPart::WHOLE;
  bool ev_general = false;   // TET4_EV: every PIHNA term (22 moments) instead of the shipped pattern (16)
};

namespace path_detail {
inline bool tet4_special(const Facts& f) { return f.nen == 4 && f.variant != RDC_VARIANT_GENERIC; }
inline bool rowgather(const Facts& f) { return f.strategy == RDC_SCATTER_ROWGATHER; }
inline Inst inst_of(const PathModel& m, const Facts& f) {
  if (f.variant == RDC_VARIANT_GENERIC || !f.opt.specialise || !f.pattern || (m.sparse_tet4_only && f.nen != 4)) return Inst::FULL;
  return m.pihna && f.opt.moments ? Inst::MOMENTS : Inst::SPARSE;
}
// k_tet4_evc serves the FULL instantiation only
inline bool evc_model(const PathModel& m, const Facts& f) { return m.evc_eligible && !(f.opt.specialise && f.pattern); }
inline bool tet4_cl_lists(const PathModel& m, const Facts& f) {
  return f.nen == 4 && (f.tet4_cl_mode == 2 || (f.tet4_cl_mode == 1 && m.cl_mode1 && !f.rg2_ok));
}
// the persistent form ("hex_kernel" = 2) assembles whole meshes only
inline bool hex8_cl_lists(const PathModel& m, const Facts& f) {
  return f.nen == 8 && (m.nv == 3 || m.nv == 5) && f.opt.hex_kernel != 1 && (f.opt.part == 0 || f.opt.hex_kernel == 0) && rowgather(f) &&
         f.opt.solid_cl_waves == 31;
}
inline bool pair_eid(const PathModel& m, const Facts& f) { return f.nlist && (m.per_elem || m.aux_local) && f.pair_eid; }
}  // namespace path_detail

// the lists this call tries to build or upload before it decides (cluster lists: at most one kind, by the element type)
inline Builds path_builds(const PathModel& m, const Facts& f) {
  using namespace path_detail;
  Builds b;
  b.pair_eid = pair_eid(m, f);
  b.ev = evc_model(m, f) && tet4_special(f) && !f.ev_tried && f.rg2_ok && f.opt.kernel == 0 && rowgather(f);
  b.tet4_cl = tet4_cl_lists(m, f);
  b.hex8_cl = hex8_cl_lists(m, f);
  return b;
}

inline Plan path_decide(const PathModel& m, const Facts& f) {
  using namespace path_detail;
  const Options& o = f.opt;
  Plan p;
  p.inst = inst_of(m, f);
  const bool special = tet4_special(f), rg = rowgather(f);
  const int kernel = (o.kernel == 5 || o.kernel == 7) ? 0 : o.kernel;   // 5 and 7 ask for what the pair cascade and the lists give anyway
  const bool tet4_cl = tet4_cl_lists(m, f) && f.cl_ready && rg && special && f.cl_fits;
  const bool hex8_cl = hex8_cl_lists(m, f) && f.cl_ready;
  // element visits: the default; the diagnostic knobs of the pair kernels select those instead
  const bool ev_lists = !tet4_cl && f.ev_ok && (o.kernel == 0 || o.kernel == 7) && o.moments && (!o.ablate || o.kernel == 7) &&
                        (!f.stamps || (o.kernel == 7 && o.ablate == 4)) && o.occupancy != 1 && o.lds_pad == 0 && special && rg;
  const bool ev_pihna = ev_lists && m.pihna && (o.ev_general || (o.specialise && f.pattern));
  const bool ev_evc = ev_lists && evc_model(m, f);
  // the instantiation that runs decides what the pair kernels need
  const bool per_elem = p.inst == Inst::FULL ? m.per_elem : m.sparse_per_elem;
  const bool plain = !per_elem && !m.aux_local;
  const bool eid = pair_eid(m, f);
  const bool rg5_lists = f.rg2_ok && f.pair_aux && f.nlist && f.rg2_block == 256;

  // first match (the table of DESIGN.md, "Which kernel runs"); a TET4 instantiation that is not plain has rg5 and coloured only
  if (tet4_cl) p.path = Path::TET4_CL;
  else if (ev_pihna) { p.path = Path::TET4_EV; p.ev_general = !(o.specialise && f.pattern); }
  else if (special && !rg) p.path = Path::TET4_COLOURED;
  else if (ev_evc && o.kernel == 0) p.path = Path::TET4_EVC;
  else if (special && rg5_lists && (plain ? kernel == 0 : eid)) p.path = Path::TET4_RG5;
  else if (special && plain && f.rg2_ok && f.pair_aux && (kernel == 0 || kernel == 3)) p.path = Path::TET4_RG3;
  else if (special && plain && f.rg2_ok && kernel == 2 && f.rg2_block == 256) p.path = Path::TET4_RG2;
  else if (special && plain) p.path = Path::TET4_ROWGATHER;
  else if (!rg) p.path = Path::GENERIC_COLOURED;
  else if (f.nen == 8 && f.rowgather_ok && hex8_cl) p.path = m.nv == 3 ? Path::HEX8_CL : Path::HEX8_CL_ROWS;
  else p.path = Path::GENERIC_ROWGATHER;

  if (o.part == 0) p.two_part = TwoPart::WHOLE;
  else if (ev_pihna || ev_evc) p.two_part = TwoPart::EV_SPLIT;
  else if (hex8_cl || tet4_cl) p.two_part = TwoPart::CL_SPLIT;
  else if (p.path == Path::TET4_RG5 && kernel == 0 && o.interior_nodes >= 0 && ((!m.per_elem && !m.aux_local) || eid)) p.two_part = TwoPart::PAIR_SPLIT;
  else p.two_part = TwoPart::ALL_IN_PART2;
  return p;
}

}  // namespace rdc
#endif
