// rdc_options.h — what rdc_set_option (include/rdc_assembly.h) sets: the tuning options of the assembly and the settings of the
// linear solve, one table each, from which the struct, the key list and the setter are generated.  Host only (no HIP): the CPU
// suite compiles it with g++ (tests/host_options_shim.cpp).
#ifndef RDC_OPTIONS_H
#define RDC_OPTIONS_H

#include <stdint.h>
#include <cstdio>
#include <cstring>

#include "../../include/rdc_assembly.h"

namespace rdc {

// One row per option: X(key = member of Options, type, default, check of an incoming value v, what is stored for v).  The check
// is RDC_ANY, or RDC_ONLY(accepted values, printf arguments of the message of a refused one).  A new option is one row here.
#define RDC_ANY
#define RDC_ONLY(accepted, ...) if (!(accepted)) { std::snprintf(err, errlen, __VA_ARGS__); return RDC_ERR_INVALID; }
#define RDC_OPTIONS(X)                                                                                                                                 \
  X(occupancy, int, 2, RDC_ANY, v)                           /* launch-bound waves per SIMD of the TET4 pair kernels */                                \
  X(ablate, int, 0, RDC_ANY, v)                              /* 1..6 remove parts of the TET4 kernels (diagnostic: the results are then wrong) */      \
  X(block, int, 256, RDC_ONLY(v == 128 || v == 256, "block must be 128 or 256"), v) /* workgroup size of the pair lists (next rdc_mesh_upload) */      \
  X(specialise, int, 1, RDC_ANY, v)                          /* allow parameter-sparsity kernel variants */                                            \
  X(lds_pad, int, 0, RDC_ANY, v)                             /* k_tet4_rg5: KB of unused LDS per workgroup (fewer co-resident workgroups) */           \
  X(stagger, int, 0, RDC_ANY, v)                             /* k_tet4_rg5: start delay of every CU's second workgroup, in 1024 cycles */              \
  X(moments, int, 1, RDC_ANY, v)                             /* shipped-pattern PIHNA/TET4 rows: 1 = moment form, 0 = coefficient form */              \
  X(interior_nodes, int64_t, -1, RDC_ANY, v)                 /* owned nodes [0, n) have no ghost node in any of their elements (two-part assembly) */  \
  X(part, int, 0, RDC_ONLY(v >= 0 && v <= 2, "part must be 0, 1 or 2"), v) /* 0 = whole mesh, 1 = workgroups of interior nodes only, 2 = the rest */   \
  X(staged, int, 1, RDC_ANY, v)                              /* HEX8 generic row gather: node table in LDS */                                          \
  X(xcd, int, 0, RDC_ANY, v)                                 /* XCD-aware workgroup order of the row-gather kernel (measured: no gain) */              \
  X(schedule, int, 1, RDC_ANY, v)                            /* LDS-conflict-aware pair schedule (next rdc_mesh_upload) */                             \
  X(grid, int, 0, RDC_ANY, v)                                /* grid size of the resident element-visit kernel (0 = its default per CU) */             \
  X(prefetch, int, 0, RDC_ANY, v)                            /* L2 prefetch distance (workgroups) of the work lists in k_tet4_rg5; 0 = off */          \
  X(solid_gather, int, 0, RDC_ANY, v ? 1 : 0)                /* two-pass, pass 2: 0 = stores staged through LDS, 1 = direct 24-byte pieces */          \
  X(solid_split, int, 1, RDC_ANY, v ? 1 : 0)                 /* two-pass, pass 1: 1 = one thread per element row, 0 = HEX8 row columns split in two */ \
  X(solid_store, int, 0, RDC_ANY, v)                         /* two-pass, pass 1 diagnostics (rdc_solid.hip: 1 = direct per-thread stores, 2 = none) */ \
  X(solid_kernel, int, 0, RDC_ONLY(v >= 0 && v <= 3, "solid_kernel must be 0 (default), 1 (coloured), 2 (two-pass) or 3 (fused cluster kernel)"), v)   \
  X(hex_kernel, int, 0, RDC_ONLY(v >= 0 && v <= 2, "hex_kernel must be 0 (cluster kernel), 1 (pair kernels) or 2 (persistent cluster kernel)"), v)     \
  X(solid_cl_order, int, -1, RDC_ANY, v < 0 ? -1 : (v ? 1 : 0)) /* pair order of the cluster lists: 1 = element-major, 0 = node-distinct, -1 = by first use */ \
  X(solid_cl_waves, int, 31, RDC_ONLY(v == 31 || v == 62, "solid_cl_waves must be 31 (3 consumer + 1 producer waves) or 62"), v)                       \
  X(ev_background, int, 1, RDC_ANY, v ? 1 : 0)               /* element-visit kernel: skip the zero moments of waves in the background state */        \
  X(ev_general, int, 1, RDC_ANY, v ? 1 : 0)                  /* PIHNA / TET4, any parameter values: 1 = element-visit kernel (22 moments), 0 = pair kernel */ \
  X(ev_resident, int, 1, RDC_ANY, v == 2 ? 2 : (v ? 1 : 0))  /* k_tet4_evq: 1 = whole-mesh launches, 2 = launches of any size, 0 = never (k_tet4_ev) */ \
  X(evc_occupancy, int, 2, RDC_ANY, v == 3 ? 3 : 2)          /* waves per SIMD of k_tet4_evc: 2, or 3 (spills: measured 2.24 vs 1.42 ms) */            \
  X(ev_occupancy, int, 3, RDC_ANY, v)                        /* waves per SIMD of the element-visit kernel: 3 (168 registers) or 2 */                  \
  X(ev_lds, int, 54000, RDC_ANY, v)                          /* LDS bytes per workgroup the element-visit clusters are sized for (next rdc_mesh_upload) */ \
  X(kernel, int, 0, RDC_ONLY(v == 0 || v == 1 || v == 2 || v == 3 || v == 5 || v == 7, "kernel must be 0, 1, 2, 3, 5 or 7, not %d", v), v) /* TET4: 1 = k_tet4_rowgather, 2 = rg2, 3 = rg3, 5 = rg5, 7 = element visits */

// The settings of the linear solve (rdc_capi_solve.hip), rows of the same shape.  The three bounds that rdc_solve.h owns stand here
// as literals (this header knows no HIP); rdc_capi_internal.h holds them to MG_OMEGA_PERMILLE, GMRES_DEFAULT_RESTART, GMRES_MAX_RESTART.
constexpr int SOLVE_OPT_MG_OMEGA = 600, SOLVE_OPT_GMRES_RESTART = 30, SOLVE_OPT_GMRES_MAX_RESTART = 128;
#define RDC_SOLVE_OPTIONS(X)                                                                                                                           \
  X(mg_omega, int, SOLVE_OPT_MG_OMEGA, RDC_ONLY(v >= 1 && v <= 1999, "mg_omega is the damping in thousandths, 1 .. 1999, not %d", v), v)               \
  X(mg_smoother, int, 0, RDC_ONLY(v == 0 || v == 1, "mg_smoother is 0 or 1, not %d", v), v)    /* 0 = damped block Jacobi, 1 = multicolour Gauss-Seidel */ \
  X(mg_gs_fuse, int, 1, RDC_ONLY(v == 0 || v == 1, "mg_gs_fuse is 0 or 1, not %d", v), v)      /* small levels sweep in one launch (0: one launch per colour everywhere) */ \
  X(ilu_factor_bits, int, 64, RDC_ONLY(v == 64 || v == 32, "ilu_factor_bits is 64 or 32, not %d", v), v) /* what the ILU(0) sweeps stream: the FP64 factor or its fp32 copy */ \
  X(solve_method, int, 0, RDC_ONLY(v == 0 || v == 1, "solve_method is 0 (BiCGStab) or 1 (GMRES), not %d", v), v) /* rdc_solve, rdc_solve_mixed */      \
  X(gmres_restart, int, SOLVE_OPT_GMRES_RESTART, RDC_ONLY(v >= 1 && v <= SOLVE_OPT_GMRES_MAX_RESTART, "gmres_restart is 1 .. %d, not %d", SOLVE_OPT_GMRES_MAX_RESTART, v), v) \
  X(gmres_refine, int, 0, RDC_ONLY(v == 0 || v == 1, "gmres_refine is 0 or 1, not %d", v), v)  /* 1 = always a second Gram-Schmidt pass */

// of a table: the struct of its members, its key list, and its setter -- what rdc_set_option does with a key of that table: RDC_OK,
// or RDC_ERR_INVALID with the message in err and o unchanged (a key of another table is unknown to it)
#define RDC_OPTION_MEMBER(key, type, def, check, store) type key = def;
#define RDC_OPTION_KEY(key, type, def, check, store) #key,
#define RDC_OPTION_SET(name, type, def, check, store) \
  if (!std::strcmp(key, #name)) {                     \
    check                                             \
    o.name = (store);                                 \
    return RDC_OK;                                    \
  }
#define RDC_OPTION_TABLE(Struct, TABLE, keys_fn, set_fn)                                           \
  struct Struct { TABLE(RDC_OPTION_MEMBER) };                                                      \
  inline const char* const* keys_fn(int* n) {                                                      \
    static const char* const keys[] = {TABLE(RDC_OPTION_KEY)};                                     \
    *n = (int)(sizeof(keys) / sizeof(keys[0]));                                                    \
    return keys;                                                                                   \
  }                                                                                                \
  inline int set_fn(Struct& o, const char* key, int value, char* err, size_t errlen) {             \
    const int v = value;                                                                           \
    TABLE(RDC_OPTION_SET)                                                                          \
    std::snprintf(err, errlen, "unknown option '%s'", key);                                        \
    return RDC_ERR_INVALID;                                                                        \
  }
RDC_OPTION_TABLE(Options, RDC_OPTIONS, option_keys, options_set)
RDC_OPTION_TABLE(SolveOptions, RDC_SOLVE_OPTIONS, solve_option_keys, solve_options_set)

inline bool solve_option_known(const char* key) {   // which table rdc_set_option asks
  int n = 0;
  const char* const* keys = solve_option_keys(&n);
  while (n > 0 && std::strcmp(key, keys[n - 1])) n--;
  return n > 0;
}

}  // namespace rdc
#endif
