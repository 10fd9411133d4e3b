/*
 * rdc_assembly.h — C-ABI of the MI355X-native element-assembly path of rdcFEs.
 *
 * This is the drop-in boundary.  Every entry point replaces a piece of
 * what the reference does inside its libMesh assemble callbacks:
 *
 *   reference (file:line, under the upstream tree)             this header
 *   ---------------------------------------------------------  ---------------------------
 *   mesh.active_local_element_ptr_range()   src/pihna.C:383     rdc_mesh_upload
 *   DofMap::dof_indices                     src/pihna.C:385-394 rdc_mesh_upload (dof = node*nvar+var)
 *   es.init() sparsity pattern              src/pihna.C:48      rdc_csr_dims / rdc_csr_pattern_download
 *   system.old_solution(dof)                src/pihna.C:433     rdc_field_upload(RDC_FIELD_OLD_SOLUTION)
 *   TD_system / RT_system.current_solution  src/ripf.C:470,477  rdc_field_upload(RDC_FIELD_AUX_NODAL)
 *   aux_system undeformed coordinates       src/solid_system.C:221-229  rdc_field_upload(RDC_FIELD_UNDEFORMED_XYZ)
 *   fibre_sys / subdomain_id                src/solid_system.C:183-216  rdc_field_upload(RDC_FIELD_ELEM_FIBRE), rdc_solid_set_materials
 *   mesh node positions (moving mesh)       src/solid_system.C:103-123  rdc_mesh_update_coords
 *   assemble_pihna                          src/pihna.C:318-758 rdc_assemble_pihna
 *   assemble_ripf                           src/ripf.C:337-673  rdc_assemble_ripf
 *   assemble_hcc                            src/coupled_hcc.C:414-649   rdc_assemble_hcc
 *   SolidSystem::element_time_derivative    src/solid_system.C:146-271  rdc_solid_assemble
 *   SolidSystem::side_time_derivative       src/solid_system.C:273-371  rdc_solid_assemble (sides set by rdc_solid_set_sides)
 *   matrix.add_matrix / rhs->add_vector     src/pihna.C:754-755 results: rdc_csr_values_device_ptr / rdc_csr_download
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns an int status (RDC_OK == 0);
 *     rdc_last_error() gives a human-readable message for the last failure on a context.
 *   - all caller buffers are caller-owned; the library copies what it needs.
 *   - one context == one GPU == one mesh partition == one system of `nvar` FIRST-LAGRANGE variables.
 *     Calls on one context are not thread-safe (the reference callback is single-threaded per rank).
 *   - DoF numbering: dof = local_node * nvar + var  (libMesh variable-group numbering).
 *   - nodes [0, n_owned_nodes) are owned: their matrix rows / rhs entries are assembled completely
 *     on this context.  Nodes [n_owned_nodes, n_nodes) are ghosts (values supplied by halo exchange).
 *     The element list must contain every element touching an owned node (owned + one ghost layer).
 *   - matrix = scalar CSR (PETSc AIJ layout) over the owned rows, column indices are LOCAL dof ids
 *     (owned and ghost), sorted ascending within a row.  Row r = node*nvar + var.
 *   - there is NO CPU fallback: without a usable HIP device rdc_ctx_create fails with RDC_ERR_HIP.
 */
#ifndef RDC_ASSEMBLY_H
#define RDC_ASSEMBLY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDC_ABI_VERSION 3   /* 2: round-2 additions (solid post-process, ADPM/PROTEAS, chunked hand-back); 3: per-part entry points, part-1 bound recorded by the call */

/* status codes */
#define RDC_OK               0
#define RDC_ERR_INVALID      1   /* bad argument (null pointer, bad size, out-of-range index) */
#define RDC_ERR_HIP          2   /* HIP runtime failure / no device */
#define RDC_ERR_STATE        3   /* call order violated (e.g. assemble before mesh upload) */
#define RDC_ERR_UNSUPPORTED  4   /* element type / model combination not implemented */
#define RDC_ERR_ALLOC        5   /* host or device allocation failed */
#define RDC_ERR_COMM         6   /* a communication callback of rdc_solve_dist returned non-zero */

/* element types (value == nodes per element) */
#define RDC_TET4 4
#define RDC_HEX8 8

/* scatter strategies */
#define RDC_SCATTER_AUTO       0  /* pick the fastest implemented for (model, element type) */
#define RDC_SCATTER_COLOURED   1  /* element-parallel, colour batches, plain read-modify-write, no atomics */
#define RDC_SCATTER_ROWGATHER  2  /* row-owner gather: every CSR value written exactly once, streaming stores */

/* kernel variants (test / benchmarking hook) */
#define RDC_VARIANT_AUTO     0  /* factored TET4 kernels where available, generic otherwise */
#define RDC_VARIANT_GENERIC  1  /* always the generic quadrature-loop kernels */

/* fields */
#define RDC_FIELD_OLD_SOLUTION   0  /* [n_nodes][nvar]   system.old_local_solution                     */
#define RDC_FIELD_AUX_NODAL      1  /* [n_nodes][naux]   RIPF: {cc_dtime, fb_dtime, RT_total}          */
#define RDC_FIELD_UNDEFORMED_XYZ 2  /* [n_nodes][3]      solid: "SolidSystem::auxiliary"               */
#define RDC_FIELD_ELEM_FIBRE     3  /* [n_elem][3]       solid: fibre direction, vars 0..2 of "::fibre" */
#define RDC_FIELD_ELEM_TRACTS    3  /* [n_elem][3]       ADPM: the "Tracts" system (src/adpm.C:448-453); same slot as the fibre */
#define RDC_FIELD_PREV_SOLUTION  4  /* [n_nodes][nvar]   RIPF check_solution: prev_soln (src/ripf.C:675,769)         */
#define RDC_FIELD_TIME_DERIV     5  /* [n_nodes][nvar]   "RIPF-TimeDeriv" system (src/ripf.C:738-740)                */
#define RDC_FIELD_RT_DOSE        6  /* [n_nodes][3]      "RT" system {broad, focus, total} (src/ripf.C:749-760)      */
#define RDC_FIELD_COUNT          7

typedef struct rdc_ctx rdc_ctx;

/* ---- parameters: POD mirrors of the string-keyed es.parameters the callbacks read ---- */

/* src/pihna.C:358-381.  necrosis_* are the RAW input values; the division by
 * cells_max_capacity (src/pihna.C:364-366) happens inside the library, as in the reference. */
typedef struct rdc_pihna_params {
  double time_step;                    /* "time_step"                   */
  double cells_min_capacity;           /* "cells_min_capacity"  Lambda_k */
  double cells_max_capacity;           /* "cells_max_capacity"  Kappa_k  */
  double cytokines_max_capacity;       /* "cytokines_max_capacity" Kappa_a */
  double cells_max_capacity_exponent;  /* "cells_max_capacity/exponent" ek */
  double necrosis_c, necrosis_h, necrosis_v;   /* "necrosis/c|h|v" */
  double diffuse_c, taxis_c;           /* "diffuse/c", "taxis/c" */
  double diffuse_h, taxis_h;           /* "diffuse/h", "taxis/h" */
  double produce_c;                    /* "produce/c" */
  double switch_c2h, switch_h2c, switch_h2n;   /* "switch/c/to/h" ... */
  double diffuse_v, taxis_v, produce_v;        /* "diffuse/v", "taxis/v", "produce/v" */
  double secrete_a_c, secrete_a_h;     /* "secrete/a/from/c|h" */
  double uptake_a_v, decay_a;          /* "uptake/a/from/v", "decay/a" */
} rdc_pihna_params;

/* src/ripf.C:377-408.  lambda_RT_r / omicro_RT_r: if 0 the reference substitutes the runtime
 * value "RT_dose/total/max" (src/ripf.C:398-403); pass that in RT_dose_total_max. */
typedef struct rdc_ripf_params {
  double time_step;
  double VolFr_stroma, VolFr_parenchyma, VolFr_exponent, VolFr_min_vacant, VolFr_max_vacant;
  double phi_cc_B, phi_cc_D, phi_cc, phi_fb_B, phi_fb_D, phi_fb, phi_tol;
  double kappa, kappa_RT_c, delta, delta_RT_a, delta_RT_b;
  double lambda, lambda_RT_r, lambda_HU_r;
  double omicro, omicro_RT_r, omicro_fb_b;
  double omega, diffusion, haptotaxis, radiotaxis;
  int32_t RT_dose_total_max;           /* es.parameters.get<int>("RT_dose/total/max") */
  int32_t _pad;
} rdc_ripf_params;

/* src/coupled_hcc.C:450-461 (necrosis_* raw; divided by cells/max_capacity inside). */
typedef struct rdc_hcc_params {
  double time_step;
  double cells_min_capacity, cells_max_capacity, cells_max_capacity_exponent;
  double produce_l;
  double diffuse_c, mechano_c, produce_c;
  double necrosis_l, necrosis_c, necrosis_pressure;
} rdc_hcc_params;

/* per-subdomain material, src/solid_system.C:183-190 */
/* es.parameters of assemble_adpm, src/adpm.C:367-413 (keys in the comments; defaults src/adpm.C:163-233).
 * pulse / sigmoid triples = {magnitude, c0, c1}, trapezoid = {magnitude, c0, c1, c2, c3} (src/utils.h:100-187). */
typedef struct rdc_adpm_params {
  double time_step;                 /* "time_step"                                             */
  double time;                      /* system.time: decay/PrP is scaled by pow(time, exponent) */
  double decay_PrP_time_exponent;   /* "decay/PrP/time_exponent"                               */
  double decay_PrP[3];              /* "decay/PrP", ".../pulse/0", ".../pulse/1"               */
  double transform_A_b[5];          /* "transform/A_b", ".../trapezoid/0..3"                   */
  double transform_Tau[5];          /* "transform/Tau", ".../trapezoid/0..3"                   */
  double diffuse_A_b[3];            /* "diffuse/A_b", ".../pulse/0,1"                          */
  double taxis1_A_b[3];             /* "taxis_1/A_b", ".../pulse/0,1"                          */
  double taxis2_A_b[3];             /* "taxis_2/A_b", ".../pulse/0,1"                          */
  double produce_A_b[3];            /* "produce/A_b", ".../sigmoid/0,1"                        */
  double decay_A_b[3];              /* "decay/A_b", ".../pulse/0,1"                            */
  double diffuse_Tau[3];            /* "diffuse/Tau", ...                                      */
  double taxis1_Tau[3];             /* "taxis_1/Tau", ...                                      */
  double taxis2_Tau[3];             /* "taxis_2/Tau", ...                                      */
  double produce_Tau[3];            /* "produce/Tau", ".../sigmoid/0,1"                        */
  double decay_Tau[3];              /* "decay/Tau", ...                                        */
  double taxis_A_b_angle;           /* "taxis/A_b/angle" in RADIANS (input() converts degrees, src/adpm.C:193) */
  double taxis_Tau_angle;           /* "taxis/Tau/angle" in radians                            */
} rdc_adpm_params;

/* es.parameters of assemble_proteas_model, src/proteas.C:376-409 (all defaults 1.0, time_step 1e-9; :135,180-212) */
typedef struct rdc_proteas_params {
  double time_step;            /* "time_step"                */
  double cells_total_capacity; /* "cells/total_capacity"     */
  double RT_max_dosage;        /* "radiotherapy/max_dosage"  */
  double host_proliferation, host_vsc_threshold, host_RT_death_rate, host_RT_exp_a, host_RT_exp_b, host_necrosis_rate;
  double tumour_diffusion, tumour_diffusion_host, tumour_proliferation, tumour_vsc_threshold, tumour_RT_death_rate,
         tumour_RT_exp_a, tumour_RT_exp_b, tumour_necrosis_rate;
  double necrosis_clearance, necrosis_slope, necrosis_vsc_threshold;
  double vascular_proliferation, vascular_necrosis_rate;
  double oedema_diffusion, oedema_proliferation, oedema_vsc_threshold, oedema_RT_coeff, oedema_RT_exp,
         oedema_reabsorption_rate;
} rdc_proteas_params;

typedef struct rdc_solid_material {
  double Young, Poisson, FibreStiffness;
  double rate[3];                      /* VolumetricStretchRatio/rate_0..2 */
} rdc_solid_material;

/* src/solid_system.C:181,234,291,306 */
typedef struct rdc_solid_params {
  double pseudo_time;                  /* "pseudo_time" */
  double displacement_penalty;         /* "BCs/displacement_penalty" */
  int32_t use_symmetry;                /* "solver/assembly_use_symmetry" */
  int32_t _pad;
} rdc_solid_params;

/* ---- context ---- */
int rdc_abi_version(void);
/* GPUs visible to this process (one MPI rank drives one of them: device_ordinal = node-local rank % count) */
int rdc_device_count(int* n_devices);
int rdc_ctx_create(int device_ordinal, rdc_ctx** out);
int rdc_ctx_destroy(rdc_ctx* ctx);
/* message for the last failing call on ctx (ctx may be NULL: last rdc_ctx_create failure) */
const char* rdc_last_error(const rdc_ctx* ctx);
/* run all work of this context on an externally created hipStream_t (NULL = default stream) */
int rdc_set_stream(rdc_ctx* ctx, void* hip_stream);
int rdc_synchronize(rdc_ctx* ctx);
int rdc_set_scatter(rdc_ctx* ctx, int strategy);
int rdc_get_scatter(const rdc_ctx* ctx, int* strategy);
int rdc_set_kernel_variant(rdc_ctx* ctx, int variant);
/* tuning / profiling knobs, not needed for normal use.  "occupancy": launch-bound waves per SIMD of
 * the TET4 row-gather kernel; "ablate": 1..6 remove parts of that kernel (results are then WRONG);
 * "moments": 1 (default) evaluates PIHNA/TET4 rows in moment form when the parameters have the shipped pattern (cell
 * transport off), 0 in coefficient form -- same sums, other association; "specialise": 0 disables that parameter-
 * pattern variant altogether; "kernel" (TET4: 0 = default, 1 = k_tet4_rowgather, 2 = k_tet4_rg2, 3 = k_tet4_rg3, 5 = k_tet4_rg5,
 * 7 = element-visit kernel; any other value is RDC_ERR_INVALID), "staged", "stagger", "prefetch", "xcd", "schedule", "block", "grid",
 * "ev_occupancy", "ev_lds", "evc_occupancy", "ev_resident" (1, default = whole-mesh launches of at least 56 clusters per resident workgroup run as three resident
 * workgroups per CU that fetch the whole next cluster by LDS-DMA while the current one is expanded and copied out, clusters handed
 * out by a counter; 2 = launches of any size; 0 = never) -- the others are experimental and
 * slower than the default -- select alternative / diagnostic kernels.  PIHNA / TET4, element-visit kernel:
 * "ev_general" 1 (default) = any parameter values through the kernel with all 22 moments, 0 = through the (node, element) pair
 * kernel as before round 3; "ev_background" 1 (default) = waves all of whose elements are in the background state of the shipped
 * field file (n = c = h = a = 0, v > 0) do not evaluate the moments and right-hand sides that are sums of exact zeros -- same
 * matrix, the kernel time then depends on the state --, 0 = everything is evaluated; "const_rows" 1 (default) = with
 * uptake/a/from/v = 0 the matrix rows of the a equation (a fifth of the values) do not depend on the unknowns, and an element-visit
 * launch that finds them in the value array from an earlier one with the same dt * secrete/a/from/c, dt * secrete/a/from/h and
 * dt * decay/a does not write them again -- the a rows of the value array PERSIST between calls: do not write over them.  The
 * library forgets them on rdc_mesh_upload, rdc_mesh_update_coords, a change of "interior_nodes", any assembly through another
 * kernel or model and a failed launch, stops skipping once rdc_csr_values_device_ptr (until the next rdc_mesh_upload) or
 * rdc_mesh_coords_device_ptr (for good) has given out a writable pointer, and always writes every row into a stream that is
 * capturing a graph; 0 = every launch writes every row; 2 = as 1, and the caller promises not to write the value or coordinate
 * arrays through the pointers it was given, which then do not stop the skipping.  HEX8 with three unknowns: "hex_kernel" 0 =
 * producer / consumer cluster kernel (default), 1 = (node, element) pair kernels, 2 = persistent form of the cluster
 * kernel; "solid_kernel" 0 = fused cluster kernel for HEX8 tangent requests and the two-pass form otherwise (default),
 * 1 = coloured read-modify-write, 2 = two-pass always (bitwise reproducible sums), 3 = fused (error when unavailable);
 * "solid_cl_waves", "solid_cl_order" = shape / pair order of the cluster lists; "solid_gather", "solid_split",
 * "solid_store" = diagnostics of the solid kernels.
 * Two-part assembly, for overlapping a halo exchange with the assembly of rows that do not need it:
 * "interior_nodes" = n states that no element of the owned nodes [0, n) contains a ghost node (the caller numbers
 * its owned nodes interior-first; set it BEFORE rdc_mesh_upload where possible: the work lists are then built so that
 * part 1 covers every interior row, otherwise only the workgroups that happen to lie inside [0, n)); with "part" = 1 an assemble call then writes only the rows of leading workgroups
 * inside [0, n), with "part" = 2 the remaining rows, with "part" = 0 (default) all rows.  Part 1 followed by part 2
 * gives exactly the matrix and residual of one whole call.  The TET4 row-gather kernels and the HEX8 cluster kernels
 * (reaction-diffusion models and the fused solid tangent; their cluster lists keep interior and near-ghost nodes apart, the
 * penalty sides of the solid system are added by part 2 behind part 1) launch sub-ranges; the paths that cannot (the
 * HEX8 pair kernels, the coloured strategy, the two-pass solid form) write nothing in part 1 and everything in part 2.
 * Stream contract: part 1 and part 2 of a step may be issued on DIFFERENT streams (rdc_set_stream in between).  Part 1
 * reads the values of owned nodes only, so the ghost rows of the bound fields may be rewritten (halo exchange)
 * while it runs; part 2 must be issued behind that exchange on its stream.  The library itself orders part 2 behind
 * part 1's preparation of the owned node data (an internal event), and neither part writes data the other may be
 * reading.  The caller orders the NEXT step's exchange behind this step's part 2 (it reads the ghost rows). */
int rdc_set_option(rdc_ctx* ctx, const char* key, int value);

/* ---- mesh / pattern (one-time set-up; replaces es.init()) ---- */
/* conn: [n_elem][elem_type] local node ids, libMesh/Gmsh node order; xyz: [n_node][3]. */
int rdc_mesh_upload(rdc_ctx* ctx, int elem_type, int64_t n_elem, int64_t n_node,
                    int64_t n_owned_nodes, const uint32_t* conn, const double* xyz, int nvar);
/* moving mesh: new CURRENT node positions (host pointer), same numbering */
int rdc_mesh_update_coords(rdc_ctx* ctx, const double* xyz);
/* device pointer of the current coordinates [n_node][3] (e.g. to update them in place on the GPU); ends the skipping of
 * "const_rows" = 1 for the life of the context (the library cannot see such updates) */
int rdc_mesh_coords_device_ptr(rdc_ctx* ctx, double** d_xyz);
int rdc_mesh_dims(const rdc_ctx* ctx, int64_t* n_elem, int64_t* n_node, int64_t* n_owned_nodes,
                  int* elem_type, int* nvar, int* n_colours);
int rdc_csr_dims(const rdc_ctx* ctx, int64_t* n_rows, int64_t* nnz);
int rdc_csr_pattern_download(const rdc_ctx* ctx, int64_t* row_ptr, int32_t* col_idx);
/* element colouring used by the coloured scatter (test hook): colour id per element */
int rdc_mesh_colours_download(const rdc_ctx* ctx, int32_t* colour_of_elem);

/* ---- fields ---- */
int rdc_field_upload(rdc_ctx* ctx, int field, const double* host, int64_t count);
int rdc_field_download(rdc_ctx* ctx, int field, double* host, int64_t count);
/* library-owned device storage of a field (allocated on first use) */
int rdc_field_device_ptr(rdc_ctx* ctx, int field, int64_t count, double** d_ptr);
/* use caller-owned device memory for a field (must stay valid until rebound / ctx destroyed) */
int rdc_field_bind_device(rdc_ctx* ctx, int field, double* d_ptr, int64_t count);

/* ---- solid-only set-up ---- */
/* subdomain index per element (index into materials[]), materials table */
int rdc_solid_set_materials(rdc_ctx* ctx, const int32_t* elem_material, int32_t n_materials,
                            const rdc_solid_material* materials);
/* boundary sides with a displacement BC: element id, libMesh side number, prescribed displacement
 * (NaN component = unconstrained, src/solid_system.C:346,358) */
int rdc_solid_set_sides(rdc_ctx* ctx, int64_t n_sides, const int64_t* side_elem,
                        const int32_t* side_id, const double* side_displacement /* [n_sides][3] */);

/* ---- the hot path: one call == one invocation of the reference's assemble callback ----
 * Pre: mesh + fields uploaded.  Post: CSR values and rhs hold the assembled sums for the owned rows
 * (the library zeroes/overwrites them itself: libMesh zeroes matrix & rhs before the callback). */
int rdc_assemble_pihna(rdc_ctx* ctx, const rdc_pihna_params* p);
int rdc_assemble_ripf(rdc_ctx* ctx, const rdc_ripf_params* p);
int rdc_assemble_hcc(rdc_ctx* ctx, const rdc_hcc_params* p);
/* assemble_adpm, src/adpm.C:324-652: unknowns PrP, A_b, Tau; needs RDC_FIELD_ELEM_TRACTS */
int rdc_assemble_adpm(rdc_ctx* ctx, const rdc_adpm_params* p);
/* assemble_proteas_model, src/proteas.C:338-705: unknowns host, tumour, necrotic, vascular,
 * oedema; RDC_FIELD_AUX_NODAL = {AUX "HU", AUX "RTD", 0} per node.  As upstream, the radiotherapy dose at a point is
 * phi_1 * (AUX variable 0 at LOCAL NODE 1 of the element) (src/proteas.C:481): only component 0 is read, and only
 * at that node of every element. */
int rdc_assemble_proteas(rdc_ctx* ctx, const rdc_proteas_params* p);
/* residual (+ Jacobian if request_jacobian) of the SolidSystem; nvar must be 3 */
int rdc_solid_assemble(rdc_ctx* ctx, const rdc_solid_params* p, int request_jacobian);
/* One part of a two-part step in ONE call: as the assemble call of the same name with "part" = part (0 = whole, 1, 2) and
 * on `hip_stream` (a hipStream_t; NULL = the default stream) for this call only -- the context's "part" option and stream
 * are left as they were.  The step of a partitioned run (src/pihna.C:801 system.update() overlapped with the assembly of
 * the interior rows) is then: rdc_assemble_pihna_part(ctx, p, 1, main); [halo exchange on side]; rdc_assemble_pihna_part(ctx, p, 2, side). */
int rdc_assemble_pihna_part(rdc_ctx* ctx, const rdc_pihna_params* p, int part, void* hip_stream);
int rdc_assemble_hcc_part(rdc_ctx* ctx, const rdc_hcc_params* p, int part, void* hip_stream);
int rdc_solid_assemble_part(rdc_ctx* ctx, const rdc_solid_params* p, int request_jacobian, int part, void* hip_stream);

/* ---- TET4 cluster kernel: the element loops src/pihna.C:383-756, src/ripf.C:410-671, src/coupled_hcc.C:463-646,
 * src/adpm.C:370-528 and src/proteas.C:338-705 on UNSTRUCTURED tetrahedral meshes (Gmsh, Delaunay: nodes with more than 16
 * node blocks in their row, for which neither the pair lists nor the element-visit lists exist).  A workgroup owns a cluster
 * of owned nodes grown over the mesh graph, gathers every element touching it once into LDS and assembles the cluster's
 * CSR rows there.  Additive: RDC_ABI_VERSION stays 3.
 *   mode 0  off (the default): nothing changes anywhere;
 *   mode 1  on where the mesh has neither element-visit lists nor pair lists, i.e. where the row-gather kernels on runs of
 *           consecutive node ids would run;
 *   mode 2  on for every TET4 mesh whose cluster lists can be built (tests, A/B against the established kernels, which
 *           are faster where they exist: DESIGN.md section 4.6).
 * Measured on a 1.17 M-tet Delaunay mesh, mode 1 against mode 0: PIHNA 1.2x, HCC 1.3x, ADPM and PROTEAS 1.9-2.0x faster, RIPF
 * equal; all five models take the kernel in mode 1.
 * Any other value: RDC_ERR_INVALID.  May be called before or after rdc_mesh_upload; on a HEX8 mesh it has no effect.  The
 * lists are built on the first assembly that wants them, honour "interior_nodes" (two-part assembly: the interior
 * clusters run in part 1) and ghosted contexts.  The kernel runs only when the scatter resolves to RDC_SCATTER_ROWGATHER
 * and the variant is not RDC_VARIANT_GENERIC; a mesh the lists cannot describe (a row of more than 255 node blocks), or an
 * image beyond the device's LDS, keeps the path it had -- rdc_last_error then carries the list builder's reason. */
int rdc_tet4_cluster_mode(rdc_ctx* ctx, int mode);
/* *active = 1 exactly if the last assembly call on this context launched the cluster kernel; the counts describe the lists
 * (0 before they exist): clusters, (owned node, element) pairs, elements gathered over all clusters; *lds_bytes = dynamic
 * LDS of that launch (0 when not active).  Any output pointer may be NULL. */
int rdc_tet4_cluster_info(rdc_ctx* ctx, int32_t* mode, int32_t* active, int64_t* n_clusters, int64_t* n_pairs,
                          int64_t* n_elem_visits, int64_t* lds_bytes);

/* ---- results ---- */
/* device pointers of the CSR values and of the rhs (either output may be NULL).  They are writable: asking for d_val
 * ends the skipping of "const_rows" = 1 until the next rdc_mesh_upload ("const_rows" = 2: the caller only reads). */
int rdc_csr_values_device_ptr(rdc_ctx* ctx, double** d_val, double** d_rhs);
int rdc_csr_download(rdc_ctx* ctx, double* val, double* rhs);
/* Chunked hand-back: the CSR values and rhs entries of the rows of nodes [node_begin, node_end) only, written to the
 * SAME positions of the full-size host arrays val / rhs as rdc_csr_download uses (either may be NULL).  async != 0:
 * the copies are only enqueued on the context's stream (use pinned host memory; complete after rdc_synchronize or an
 * event of the caller) -- so the rows of part 1 of a two-part assembly can travel while part 2 is still computing. */
int rdc_csr_download_rows(rdc_ctx* ctx, int64_t node_begin, int64_t node_end, double* val, double* rhs, int async);
/* Pipelined hand-back (src/pihna.C:754-755 hands Ke/Fe to PETSc element by element; here whole row ranges travel while the
 * device keeps assembling): as rdc_csr_download_rows, but the copies run on a stream of the context's own, behind the work
 * ENQUEUED SO FAR on the context's stream and independent of anything enqueued later -- the rows of part 1 of a two-part
 * assembly, or of the first node ranges of any assembly, are inserted into the PETSc matrix while the next chunk is in flight.
 * *ticket identifies the call; rdc_ticket_wait blocks the host until that chunk is in host memory (at most 16 calls in flight).
 * Pin the destination arrays once (rdc_host_pin: hipHostRegister) or the copies are staged and serialise. */
int rdc_csr_download_rows_async(rdc_ctx* ctx, int64_t node_begin, int64_t node_end, double* val, double* rhs, int* ticket);
int rdc_ticket_wait(rdc_ctx* ctx, int ticket);
int rdc_host_pin(rdc_ctx* ctx, void* host_ptr, size_t bytes);
int rdc_host_unpin(rdc_ctx* ctx, void* host_ptr);
/* two-part assembly: the rows of nodes [0, *n_nodes) are complete after "part" = 1 (whole workgroups inside the
 * interior; 0 when the active kernel path cannot launch sub-ranges).  After a part-1 assemble call the value is what
 * THAT call completed -- the kernel path, and with it the split, depends on the model, the parameter values and the
 * tuning options; before any part-1 call since the upload it is the prediction for a shipped-pattern PIHNA call with the
 * current scatter strategy, kernel variant, cluster mode and tuning options, on the lists the mesh has at that moment (the
 * call's own decision; it builds nothing, so lists that only the first assembly builds are not counted on). */
int rdc_part1_nodes(const rdc_ctx* ctx, int64_t* n_nodes);

/* ---- device-resident linear solve: what the reference does in model.solve() (src/pihna.C:80) and in the Newton /
 * linear solver of the solid system (src/solid_system.C:98-100,380), without handing the matrix back to the host.
 * Additive: RDC_ABI_VERSION stays 3, nothing above changes meaning.
 * The matrix is the context's own CSR values, walked through the node-block pattern (4 bytes of index per nvar x nvar
 * block, no scalar row_ptr / col_idx on the device).  BiCGStab, LEFT-preconditioned by node-block Jacobi: it iterates on
 * D^-1 A x = D^-1 b and stops on the preconditioned residual, as PETSc's KSPBCGS does by default.  rdc_solve and rdc_solve_mixed
 * take a single partition; rdc_solve_dist (below) is the same iteration across partitions. */
#define RDC_PRECOND_NONE 0
#define RDC_PRECOND_JACOBI 1
#define RDC_PRECOND_BLOCK_JACOBI 2      /* default choice of the Python wrapper */
#define RDC_PRECOND_MULTIGRID 3         /* block Jacobi's system, with an aggregation-multigrid cycle applied from the right (below) */
#define RDC_PRECOND_ILU0 4              /* block Jacobi's system, with a multicolour block ILU(0) applied from the right (below); rdc_solve only */
#define RDC_PRECOND_ILU0_LOCAL 5        /* the same with the ILU(0) of the rank's owned square: block Jacobi between the ranks, ILU(0) inside each (below); rdc_solve_dist, and rdc_solve without ghosts */
#define RDC_PRECOND_MULTIGRID_GS_LOCAL 6 /* the cycle of RDC_PRECOND_MULTIGRID with the rank-local multicolour Gauss-Seidel smoother (below); rdc_solve_dist_mg, rdc_solve_dist_gmres, and rdc_solve without ghosts */

#define RDC_SOLVE_CONVERGED     0
#define RDC_SOLVE_MAX_ITS       1       /* x holds the last iterate */
#define RDC_SOLVE_BREAKDOWN     2       /* restarts exhausted */
#define RDC_SOLVE_BAD_DIAGONAL  3       /* singular / non-finite diagonal (block); x untouched */
#define RDC_SOLVE_NOT_FINITE    4       /* rhs, x0 or the iteration produced NaN/inf; x holds the last finite iterate or x0 (an entry whose update would overflow keeps its value) */

typedef struct rdc_solve_params {
  double rel_tol;        /* stop when ||D^-1 (b - A x)|| <= max(rel_tol * ||D^-1 b||, abs_tol); D = the preconditioner */
  double abs_tol;
  double rhs_scale;      /* b = rhs_scale * (assembled rhs): 1 for the reaction-diffusion systems, -1 for a Newton update */
  int32_t max_its;
  int32_t precond;       /* RDC_PRECOND_* */
} rdc_solve_params;

typedef struct rdc_solve_info {
  int32_t reason;        /* RDC_SOLVE_* */
  int32_t iterations;    /* BiCGStab iterations = pairs of matrix-vector products, restarts included; with "solve_method" = 1 (below): Arnoldi steps = operator applications inside the GMRES cycles, bounded by max_its */
  int32_t restarts;      /* BiCGStab: recomputations of the true residual that did not end the solve; GMRES: cycles begun after the first */
  int32_t bad_blocks;    /* diagonal blocks the preconditioner could not invert */
  double rhs_norm;       /* ||D^-1 b||_2 */
  double residual_norm;  /* TRUE ||D^-1 (b - A x)||_2 of the returned x: the quantity the stopping test is about */
  double plain_rhs_norm, plain_residual_norm;   /* the same without D^-1 */
  float  device_ms;      /* device time of the whole solve (HIP events on the context stream) */
  int32_t matrix_bits;   /* width of the matrix values the ITERATION streamed: 64 (rdc_solve, or rdc_solve_mixed that fell back), 32 (rdc_solve_mixed) */
} rdc_solve_info;

/* y[n_owned*nvar] = A * x[n_nodes*nvar], both DEVICE pointers; enqueued on the context's stream, does not synchronise.
 * x covers owned and ghost dofs (local numbering), so a partitioned caller can exchange the ghosts and then multiply.
 * d_x and d_y must not overlap. */
int rdc_csr_matvec(rdc_ctx* ctx, const double* d_x, double* d_y);
/* Solve A x = rhs_scale * rhs for the values and rhs the last assemble call left in the context.
 * d_x: DEVICE pointer, n_owned*nvar doubles: initial guess on entry (libMesh hands KSP the current solution), solution on exit.
 * It may be the storage of RDC_FIELD_OLD_SOLUTION (rdc_field_device_ptr): matrix and rhs are not re-read from the fields.
 * Blocks the host until done.  Never modifies the CSR values or the rhs.
 * A solver outcome other than convergence is not an error status: the call returns RDC_OK and info->reason tells.
 * b = 0 gives x = 0 in 0 iterations.  RDC_ERR_UNSUPPORTED when the context has ghost nodes (a solve across partitions
 * needs a halo exchange of the search directions inside every iteration: rdc_solve_dist). */
int rdc_solve(rdc_ctx* ctx, const rdc_solve_params* p, double* d_x, rdc_solve_info* info);

/* ---- mixed precision (additive, RDC_ABI_VERSION stays 3): BiCGStab that iterates on an FP32 copy of D^-1 A.
 * The copy is built from the current CSR values (4 bytes per value in a layout private to the library, behind the same
 * 4-byte block index; allocated at the first use on a mesh, freed with the mesh).  Vectors, dot products and every sum
 * stay FP64.  Everything that decides or reports -- the first residual, each confirmation of a claimed convergence and
 * each restart, the closing residual, the norms in rdc_solve_info -- is computed from the FP64 values, so the returned
 * x satisfies the same inequality as that of rdc_solve; only the path to it differs.
 *
 * rdc_solve_mixed: the contract of rdc_solve.  d_x: DEVICE pointer, n_owned*nvar doubles: initial guess on entry,
 * solution on exit; may be the storage of RDC_FIELD_OLD_SOLUTION.  Blocks the host until done.  Never modifies the CSR
 * values or the rhs.  A solver outcome other than convergence is not an error status: RDC_OK and info->reason tells.
 * b = 0 gives x = 0 in 0 iterations; RDC_SOLVE_BAD_DIAGONAL leaves x untouched; RDC_ERR_UNSUPPORTED when the context
 * has ghost nodes.  It rebuilds the FP32 copy from the current values at every call.  If an entry of D^-1 A is not
 * finite in FP32, the call iterates on the FP64 values instead and returns exactly what rdc_solve returns;
 * info->matrix_bits says which happened. */
int rdc_solve_mixed(rdc_ctx* ctx, const rdc_solve_params* p, double* d_x, rdc_solve_info* info);
/* Builds D^-1 (precond: RDC_PRECOND_*) and the FP32 copy of D^-1 A from the current values.  Enqueued on the context's
 * stream, then synchronises to read its counters: RDC_ERR_INVALID, with a message, if a diagonal block is not invertible
 * or an entry is not finite in FP32 (there is no usable copy then).  Works with ghost nodes: the rows are the owned ones. */
int rdc_csr_scale_f32(rdc_ctx* ctx, int precond);
/* y[n_owned*nvar] = fl32(D^-1 A) * x[n_nodes*nvar] with the copy the last rdc_csr_scale_f32 or rdc_solve_mixed on this
 * mesh built; both DEVICE pointers, FP64.  The copy holds the values AS THEY WERE WHEN IT WAS BUILT: a later assemble call
 * does not update it.  RDC_ERR_INVALID if this mesh has no copy.  Enqueued on the context's stream, does not
 * synchronise.  d_x and d_y must not overlap. */
int rdc_csr_matvec_f32(rdc_ctx* ctx, const double* d_x, double* d_y);

/* ---- RDC_PRECOND_MULTIGRID (rdc_solve and rdc_solve_mixed; additive: RDC_ABI_VERSION stays 3) ----
 * The iteration runs on the system of RDC_PRECOND_BLOCK_JACOBI, D^-1 A x = D^-1 b, and a V(1,1) cycle M of an aggregation
 * multigrid is applied from the RIGHT: the operator of the iteration is D^-1 A M, x advances along M p and M s.  The
 * residual of the recurrence therefore stays D^-1 (b - A x): the stopping test, rel_tol / abs_tol, the confirmation of a
 * claimed convergence on the true residual, the restarts and every field of rdc_solve_info mean exactly what they mean
 * for RDC_PRECOND_BLOCK_JACOBI; only the number of iterations differs.
 * Levels: aggregates of at most 8 nodes of the node-block graph (built on the host at the first multigrid solve on a mesh,
 * deterministic), a piecewise-constant prolongation per unknown, Galerkin coarse matrices P^T A_l P in the node-block
 * layout (FP64 in both entry points, rebuilt from the current values by every solve), damped block Jacobi as the smoother
 * and, with 8 sweeps, on the last level.  The damping is the option "mg_omega" of rdc_set_option, in thousandths
 * (default 600 = 0.6; accepted 1 .. 1999).  A singular or non-finite diagonal block on ANY level counts into bad_blocks
 * and gives RDC_SOLVE_BAD_DIAGONAL with x untouched.  RDC_ERR_UNSUPPORTED with ghost nodes, and if a level would have
 * 2^31 node blocks or more.  rdc_solve_mixed streams the fp32 copy on level 0 inside the cycle as well.
 * Smoother: the option "mg_smoother" (0 or 1, default 0; anything else is RDC_ERR_INVALID and changes nothing).  With 1 the
 * first sweep from zero on every level stays x = w D_l^-1 r, and every other sweep -- the post-smoothing of every level and
 * the 7 further sweeps of the last one -- is one forward Gauss-Seidel sweep x_n += D_l^-1 (r_n - (A_l x)_n) in a
 * multicolour order, undamped.  The colours are greedy (nodes ascending, the smallest colour no coloured row neighbour
 * holds; as many colours as it takes), built on the host at the first such solve on a mesh and kept with it: 4 bytes per
 * node and level in an allocation of their own, which rdc_solve_mg_stats does not count.  A sweep reads the matrix once,
 * as a Jacobi sweep does, and takes one launch per colour; a level of at most 512 nodes sweeps in one launch of one
 * workgroup (option "mg_gs_fuse", default 1; 0 = one launch per colour on every level; the results are bitwise equal).
 * Deterministic: two solves return the same bytes.  RDC_ERR_UNSUPPORTED, with nothing launched, if the block pattern of a
 * level is not structurally symmetric (two coupled nodes would share a colour), on a context with ghost nodes, and in
 * rdc_solve_dist_mg.  With "mg_smoother" = 0 every call launches what it launched before the option existed. */
/* The hierarchy of the last multigrid solve on this mesh: *n_levels = its levels (the matrix itself is level 0), and for
 * the first min(*n_levels, cap) of them nodes[l] and blocks[l] (node blocks of the level's matrix).  nodes / blocks may
 * be NULL with cap = 0.  RDC_ERR_STATE if no multigrid solve has run on this mesh. */
int rdc_solve_mg_levels(rdc_ctx* ctx, int32_t* n_levels, int64_t* nodes, int64_t* blocks, int cap);
/* What the hierarchy costs: *setup_ms = device time the last multigrid solve spent on the Galerkin products and the D_l^-1
 * (part of its rdc_solve_info.device_ms); *level_bytes = device memory the levels hold for this mesh (matrices, lists and
 * vectors).  Either pointer may be NULL.  RDC_ERR_STATE as above. */
int rdc_solve_mg_stats(rdc_ctx* ctx, float* setup_ms, int64_t* level_bytes);
/* The colours of the Gauss-Seidel smoother: n_colours[l] for the first min(levels, cap) levels of the hierarchy
 * (rdc_solve_mg_levels tells how many there are).  RDC_ERR_STATE if no multigrid solve with "mg_smoother" = 1 has run on
 * this mesh. */
int rdc_solve_mg_colours(rdc_ctx* ctx, int32_t* n_colours, int cap);
/* ---- two read-only observation points of the cycle (additive: RDC_ABI_VERSION stays 3).  TEST HOOKS: they exist so that a
 * test can hold the cycle M and the coarse matrices to a reference; no solver path needs them, and nothing is claimed about
 * their speed.
 * rdc_solve_mg_apply: d_out = M d_in, ONE cycle, as the next rdc_solve (mixed == 0) or rdc_solve_mixed (mixed != 0) with
 * RDC_PRECOND_MULTIGRID would apply it: the call first does what such a solve does before its first iteration (D^-1, the
 * fp32 copy if mixed, the values and D_l^-1 of every level from the current CSR values -- the same host function, so the
 * hierarchy and the colours are built at first use here too), then applies the cycle in the form that solve would iterate
 * in: on the fp32 copy of level 0 if mixed and every entry of D^-1 A is finite in FP32, on the FP64 values otherwise.
 * "mg_omega", "mg_smoother" and "mg_gs_fuse" are honoured; it launches no kernel a solve does not launch.  d_in, d_out:
 * DEVICE pointers, n_owned*nvar doubles each, not overlapping.  Blocks the host until done; never modifies the CSR values
 * or the rhs.  RDC_ERR_STATE without a mesh, RDC_ERR_INVALID for a null pointer, RDC_ERR_UNSUPPORTED on a context with
 * ghost nodes (the message of rdc_solve); RDC_ERR_INVALID, with the count in the message and d_out untouched, if a
 * diagonal block of any level is not invertible. */
int rdc_solve_mg_apply(rdc_ctx* ctx, int mixed, const double* d_in, double* d_out);
/* What the last rdc_solve_mg_apply, or the last rdc_solve / rdc_solve_mixed with RDC_PRECOND_MULTIGRID, built for `level`
 * (0 .. levels - 1, rdc_solve_mg_levels), into HOST arrays: val = the level's matrix, blocks[level] * nvar^2 doubles in the
 * node-block layout of the CSR values ([var a][block k][var b] per node, over the level's own pattern); dinv = its D_l^-1,
 * nodes[level] * nvar^2 doubles, row-major per node.  Level 0 is the matrix itself: val must be NULL there, and dinv
 * receives the solver's D^-1.  Either pointer may be NULL to skip that array.  RDC_ERR_STATE if neither producer has run
 * on this mesh, or if a call that runs or plans a solve (any other rdc_solve* entry but the three queries above) or
 * rdc_csr_scale_f32 has come after it: those write over the D^-1 this call reads.  RDC_ERR_INVALID for a level out of range. */
int rdc_solve_mg_level_download(rdc_ctx* ctx, int level, double* val, double* dinv);

/* ---- RDC_PRECOND_ILU0 (rdc_solve; additive: RDC_ABI_VERSION stays 3) ----
 * The iteration runs on the system of RDC_PRECOND_BLOCK_JACOBI, D^-1 A x = D^-1 b, and M = (LU)^-1 is applied from the RIGHT,
 * exactly as the multigrid cycle is: LU is the block ILU(0) factorisation of A^ = D^-1 A on the node-block pattern.  The
 * stopping test, the confirmation of a claim on the true residual, the restarts and every field of rdc_solve_info mean what
 * they mean for RDC_PRECOND_BLOCK_JACOBI; only the number of iterations differs.
 * Elimination order: (colour, node id), the colours being the greedy ones of the Gauss-Seidel smoother on the matrix itself
 * (nodes ascending, the smallest colour no coloured row neighbour holds), built on the host at the first such solve on a mesh
 * and kept with it.  L has identity diagonal blocks, U carries the diagonal blocks, and U_ii^-1 is kept per node.  A node of
 * colour c depends on nodes of other colours only, so the factorisation is one launch per colour and each triangular sweep
 * one launch per colour: forward z_i = y_i - sum_{colour(k) < c} L_ik z_k over the colours ascending, backward
 * z_i = U_ii^-1 (z_i - sum_{colour(j) > c} U_ij z_j) descending.  The factor is rebuilt from the current values by every
 * solve; it lives in a copy of A^ (8 bytes per non-zero, 4 bytes per node block of index, in a layout private to the library,
 * allocated at the first such solve on a mesh and freed with it: rdc_solve_ilu_stats), which the two sweeps of an apply
 * together read once.  Deterministic: the order of every sum is fixed, there are no atomics, two solves return the same bytes.
 * A diagonal block of A, or a pivot U_ii, that is singular or not finite counts into bad_blocks and gives
 * RDC_SOLVE_BAD_DIAGONAL with x untouched and no iteration run.  RDC_ERR_UNSUPPORTED, with nothing launched: on a context with
 * ghost nodes, for a block pattern that is not structurally symmetric or lacks a diagonal block, and for this value of
 * precond in rdc_solve_mixed (unless "ilu_factor_bits" is 32, below), rdc_solve_dist and rdc_solve_dist_mg (across ranks: RDC_PRECOND_ILU0_LOCAL below, the rank-local
 * factor; an ILU coupled across ranks is not implemented).  Every other call launches what it launched before the value existed. */
/* What the factor costs: *setup_ms = device time the last solve (or rdc_solve_ilu_apply) spent on the copy of A^ and the
 * factorisation (part of its rdc_solve_info.device_ms); *bytes = device memory the factor holds for this mesh (values, U_ii^-1,
 * index lists, colour lists and the two vectors M p and M s); *n_colours = the colours.  Any pointer may be NULL.
 * RDC_ERR_STATE if no such solve has run on this mesh. */
int rdc_solve_ilu_stats(rdc_ctx* ctx, float* setup_ms, int64_t* bytes, int32_t* n_colours);
/* ---- the fp32 factor (option "ilu_factor_bits", rdc_set_option; additive: RDC_ABI_VERSION stays 3) ----
 * "ilu_factor_bits" is 64 (default) or 32; any other value is RDC_ERR_INVALID and changes nothing.  With 64 every entry launches,
 * returns and refuses what is described above and below.  With 32 the factorisation is unchanged (FP64, the private layout); a
 * further kernel then rounds the lower and the upper blocks to fp32 into a third allocation (made at the first solve or hook
 * with the option at 32 on a mesh, freed with the mesh, counted by rdc_solve_ilu_stats from then on: 4 bytes per off-diagonal
 * non-zero, every row of a node's lower and upper run padded to a multiple of 16 bytes, 8 bytes per node of offsets, no slot
 * for a diagonal or a ghost block), and the two sweeps of every apply stream that copy.  U_ii^-1, z, every sum and the epilogue
 * stay FP64: each value is converted to double and fed to an fma.  The set-up time of rdc_solve_ilu_stats includes the rounding.
 * Accepted with 32, beside what 64 accepts: RDC_PRECOND_ILU0 and RDC_PRECOND_ILU0_LOCAL in rdc_solve_mixed, and
 * RDC_PRECOND_ILU0_LOCAL in rdc_solve_dist with mixed != 0 (the fp32 operator with the fp32 factor).  Every other refusal stays.
 * Fall-back: the rounding counts the entries that are finite in FP64 and not in fp32, and the host reads the count with the
 * record of bad_blocks before the first iteration (no further synchronisation).  If it is not zero the sweeps stream the FP64
 * factor, and the call is bit for bit the one with the option at 64.  This is independent of the operator's fall-back
 * (matrix_bits), and across ranks each rank decides alone: M is block-diagonal over the ranks, so a mixture is a legal
 * preconditioner, and the exchanges and all-reduces per iteration stay what they are.  Deterministic as the FP64 sweeps.
 * rdc_solve_ilu_apply and rdc_solve_ilu_local_apply apply what the next solve would; the two downloads return the FP64 factor
 * the copy was rounded from.
 * rdc_solve_ilu_factor_bits: *bits = what the sweeps of the last ILU(0) solve or apply hook on this mesh streamed, 32 or 64.
 * RDC_ERR_STATE before any has run. */
int rdc_solve_ilu_factor_bits(rdc_ctx* ctx, int32_t* bits);
/* ---- two read-only observation points (additive: RDC_ABI_VERSION stays 3).  TEST HOOKS, as the multigrid pair above.
 * rdc_solve_ilu_apply: d_out = M d_in, ONE application, as the next rdc_solve with RDC_PRECOND_ILU0 would apply it: the call
 * first does what such a solve does before its first iteration (D^-1, the copy of A^, the factorisation from the current CSR
 * values -- the same host function, so colours and lists are built at first use here too).  d_in, d_out: DEVICE pointers,
 * n_owned*nvar doubles each, not overlapping.  Blocks the host until done; never modifies the CSR values or the rhs.
 * RDC_ERR_STATE without a mesh, RDC_ERR_INVALID for a null pointer, RDC_ERR_UNSUPPORTED as the solve; RDC_ERR_INVALID, with
 * the count in the message and d_out untouched, if a diagonal block or a pivot is not invertible. */
int rdc_solve_ilu_apply(rdc_ctx* ctx, const double* d_in, double* d_out);
/* The factor the last rdc_solve_ilu_apply or solve with RDC_PRECOND_ILU0 built, into HOST arrays, in the PUBLIC node-block
 * layout of the CSR values whatever the private layout is: val = nnz doubles, the L blocks and the U blocks (diagonal blocks
 * included) in the positions of the blocks they replace, the identity of L not stored; uinv = U_ii^-1, n_owned * nvar^2
 * doubles, row-major per node.  Either pointer may be NULL.  RDC_ERR_STATE if neither producer has run on this mesh. */
int rdc_solve_ilu_download(rdc_ctx* ctx, double* val, double* uinv);

/* ---- RDC_PRECOND_ILU0_LOCAL (rdc_solve_dist, FP64; additive: RDC_ABI_VERSION stays 3) ----
 * The rank-local form of RDC_PRECOND_ILU0, a preconditioner of its own: what PETSc runs by default under mpirun, block Jacobi
 * between the ranks with ILU(0) inside each.  System, stopping test and rdc_solve_info are those of RDC_PRECOND_BLOCK_JACOBI,
 * M = (LU)^-1 is applied from the right, and LU is the multicolour block ILU(0) described above of the OWNED SQUARE of A^ = D^-1 A:
 * the rows and columns below n_owned, the blocks in ghost columns left out.  The greedy colours are taken over the owned nodes in
 * local order.  With more than one rank this is another operator than that of RDC_PRECOND_ILU0 (the couplings across partitions
 * are dropped from the factor, not from the system), which is why it has a value of its own; RDC_PRECOND_ILU0 keeps its refusals.
 *   rdc_solve_dist, mixed == 0   accepted on a context with or without ghosts, with the plain rdc_solve_comm.  An apply needs no
 *                                communication: per iteration the call makes the two exchanges (of M p and M s, where block Jacobi
 *                                exchanges p and s; the rows below "interior_nodes" still run before the ghosts arrive) and the three
 *                                all-reduces of RDC_PRECOND_BLOCK_JACOBI, plus one of each per true residual -- no more.  The pivots
 *                                U_ii that could not be inverted count into bad_blocks, which rides over the ranks in the all-reduce
 *                                of the first true residual as it always has: on a bad pivot on any rank every rank returns
 *                                RDC_SOLVE_BAD_DIAGONAL with the same bad_blocks, the owned rows of x untouched and no iteration run.
 *                                On return the ghost rows of x hold the owners' values; two solves return the same bytes; a context
 *                                without ghosts and a communicator of world size 1 returns, bit for bit, what rdc_solve returns
 *                                with RDC_PRECOND_ILU0.
 *   rdc_solve, no ghosts         accepted: the owned square is the matrix, and the call returns the bytes (x and every field of
 *                                rdc_solve_info) of RDC_PRECOND_ILU0.  With ghosts it refuses as it does for every value.
 *   rdc_solve_mixed, and rdc_solve_dist with mixed != 0   RDC_ERR_UNSUPPORTED: the factor is FP64 only -- unless the option
 *                                "ilu_factor_bits" is 32 (above): the sweeps then stream the fp32 copy of the factor.
 *   rdc_solve_dist_mg            RDC_ERR_INVALID, as for anything but RDC_PRECOND_MULTIGRID.
 * The factor shares the lists and the two allocations of RDC_PRECOND_ILU0 (rdc_solve_ilu_stats serves both).  On a context with
 * ghost nodes every node block in a ghost column keeps an unused slot of nvar^2 doubles in the value buffer, the lists grow by 4
 * bytes per owned node, and M p and M s by a ghost tail; on a context without ghosts the allocations are byte for byte those of
 * RDC_PRECOND_ILU0.  RDC_ERR_UNSUPPORTED, as there, for an owned square that is not structurally symmetric or lacks a diagonal
 * block; that refusal is taken by the rank alone, before its first callback.  Out of scope: an fp32 U_ii^-1, an ILU coupled
 * across ranks, overlapping partitions. */
/* ---- RDC_PRECOND_MULTIGRID_GS_LOCAL (rdc_solve_dist_mg, rdc_solve_dist_gmres; additive: RDC_ABI_VERSION stays 3) ----
 * RDC_PRECOND_MULTIGRID across ranks with the sweeps of "mg_smoother" = 1, a preconditioner of its own: Gauss-Seidel inside each
 * rank, Jacobi between the ranks.  System, stopping test, norms, rdc_solve_info, the V(1,1) cycle from the right, the rank-local
 * aggregates, the Galerkin levels and "mg_omega" are those of RDC_PRECOND_MULTIGRID.  The first sweep from zero on every level stays
 * x = w D_l^-1 r; every other sweep is one undamped forward sweep x_n += D_l^-1 (r_n - (A_l x)_n) over this rank's own colour lists
 * of the level (the greedy colours of the owned square: columns in the ghost layer are ignored), preceded by the exchange of x on
 * that level.  During a sweep a ghost column reads the value that exchange received and is never written.  With more than one rank
 * this is another operator than the sweep of "mg_smoother" = 1 on one partition (a coupling across partitions takes the old value),
 * which is why it has a value of its own; RDC_PRECOND_MULTIGRID keeps every behaviour it has, its refusal of "mg_smoother" = 1
 * across ranks included.  "mg_smoother" is not consulted under this value (0 and 1 return the same bytes); "mg_gs_fuse" and
 * "mg_omega" are honoured, and "mg_gs_fuse" = 0 and 1 return the same bytes.
 *   rdc_solve_dist_mg            accepted beside RDC_PRECOND_MULTIGRID, FP64 and mixed (level 0 then sweeps on the fp32 copy; after
 *                                the FP32-overflow fall-back on the FP64 values).  The callbacks of the set-up and of an iteration
 *                                are exactly those of RDC_PRECOND_MULTIGRID, at every world size: the smoother costs no message.  On
 *                                level 0 the nodes of colour 0 below "interior_nodes" are swept between exchange_begin and
 *                                exchange_end.  A rank that owns no node of a level launches nothing there and makes every callback.
 *   rdc_solve_dist_gmres, rdc_solve_dist_gmres_arnoldi   accepted through the sized pair, as RDC_PRECOND_MULTIGRID is.
 *   rdc_solve, rdc_solve_mixed, rdc_solve_gmres_arnoldi, no ghosts   accepted: the call returns the bytes (x and every field of
 *                                rdc_solve_info) of RDC_PRECOND_MULTIGRID under "mg_smoother" = 1, under both methods.  With ghosts
 *                                it refuses as it does for every value.
 *   rdc_solve_dist               RDC_ERR_UNSUPPORTED naming rdc_solve_dist_mg, as for RDC_PRECOND_MULTIGRID.
 *   rdc_solve_mg_apply           takes no preconditioner; on a context with ghosts it refuses as before.
 * A context without ghosts and a communicator of world size 1 returns, bit for bit, what rdc_solve returns with
 * RDC_PRECOND_MULTIGRID under "mg_smoother" = 1.  Two solves return the same bytes (no atomics, no counters).
 * rdc_solve_mg_colours after such a partitioned solve reports THIS RANK's colours per level.  The lists share the allocation of
 * "mg_smoother" = 1: a mesh holds one set.  Those of a partitioned hierarchy are dropped whenever that hierarchy is (a new plan, new
 * peer counts, a multigrid solve on one partition, a mesh upload) and are built again by the next solve with this value; a
 * single-partition solve with "mg_smoother" = 1 afterwards colours its own hierarchy again and returns what it always did.
 * RDC_ERR_UNSUPPORTED if the owned square of a level of this rank is not structurally symmetric.  That refusal is taken by the rank
 * alone and is NOT collective: it comes behind the collective set-up of the levels and before the first callback of the solve, so
 * the other ranks must not be left waiting on it (a caller that cannot rule it out checks the return on every rank).  Out of
 * scope: a smoother coupled across ranks, the level-0 pack folded into the sweep, overlap beyond colour 0. */
/* ---- two read-only observation points that accept a context with ghost nodes (TEST HOOKS, as the pair above, which keep refusing one).
 * rdc_solve_ilu_local_apply: d_out = M d_in, ONE application of this rank's M, as the next rdc_solve_dist with
 * RDC_PRECOND_ILU0_LOCAL would apply it (the same host function: D^-1, the copy of the owned square of A^, its factorisation from
 * the current CSR values; lists built at first use).  d_in, d_out: DEVICE pointers, n_owned*nvar doubles each, not overlapping.
 * No communication.  Blocks the host until done; never modifies the CSR values or the rhs.  RDC_ERR_STATE without a mesh,
 * RDC_ERR_INVALID for a null pointer; RDC_ERR_INVALID, with the count in the message and d_out untouched, if a diagonal block or a
 * pivot of THIS rank is not invertible. */
int rdc_solve_ilu_local_apply(rdc_ctx* ctx, const double* d_in, double* d_out);
/* The factor the last rdc_solve_ilu_local_apply or solve with RDC_PRECOND_ILU0_LOCAL (or, without ghosts, RDC_PRECOND_ILU0) built,
 * into HOST arrays.  val: the layout of a node-block CSR RESTRICTED TO THE OWNED COLUMNS.  Node n has own[n] = the blocks of its row
 * whose column is below n_owned -- the leading own[n] blocks of the row, since ghost ids lie above every owned id and the columns
 * ascend; its values start at nvar^2 * (own[0] + .. + own[n - 1]) and lie as [var a][block k][var b], k = 0 .. own[n) - 1: the L
 * and U blocks (diagonal blocks included) in the positions of the blocks they replace, the identity of L not stored.  The buffer
 * is compact, nvar^2 * sum(own) doubles: it has no position for a ghost block.  Without ghosts this is the layout and content of
 * rdc_solve_ilu_download.  uinv = U_ii^-1, n_owned * nvar^2 doubles, row-major per node.  Either pointer may be NULL.
 * RDC_ERR_STATE if no producer has run on this mesh. */
int rdc_solve_ilu_local_download(rdc_ctx* ctx, double* val, double* uinv);

/* ---- restarted GMRES(m) next to BiCGStab (rdc_solve and rdc_solve_mixed; additive: RDC_ABI_VERSION stays 3) ----
 * Three solver settings of rdc_set_option choose the Krylov method of the two single-partition entries:
 *   "solve_method"   0 = BiCGStab (the default: everything above), 1 = GMRES; any other value is RDC_ERR_INVALID
 *   "gmres_restart"  1 .. 128, default 30 (PETSc's default); outside that range RDC_ERR_INVALID
 *   "gmres_refine"   0 = one classical Gram-Schmidt pass per step (PETSc's default), 1 = always a second pass (CGS2)
 * With "solve_method" = 1 the two entries run right-preconditioned GMRES(m) on the same system D^-1 A x = D^-1 b (D by precond 0, 1,
 * 2; block Jacobi for 3, 4, 5) with the same right preconditioner M (none, the multigrid cycle, the ILU(0) sweeps): what PETSc's
 * KSPGMRES does by default.  The stopping test, rhs_scale, the reasons and every guarantee above carry over: RDC_SOLVE_BAD_DIAGONAL
 * leaves x untouched, b = 0 gives x = 0, no NaN or inf is ever written into x, and residual_norm is the TRUE ||D^-1 (b - A x)|| of
 * the returned x: every cycle starts from, and ends with, the FP64 residual of x, which alone decides.  iterations counts Arnoldi
 * steps (a cycle always takes at least one), restarts the cycles begun after the first.  RDC_SOLVE_BREAKDOWN: the operator is
 * singular on the Krylov space.  Deterministic: no floating-point atomics, two solves return the same bytes.
 * The state (restart + 1 basis vectors of n_owned * nvar doubles, and a few KB) is an allocation of its own, made at the first GMRES
 * solve on a mesh, remade when "gmres_restart" grows, freed with the mesh; RDC_ERR_ALLOC with the byte count if it cannot be made.
 * With "solve_method" = 0 nothing of it is allocated, launched or read.
 * rdc_solve_dist and rdc_solve_dist_mg return RDC_ERR_UNSUPPORTED under "solve_method" = 1, before any callback is called and with
 * x untouched: allreduce_sum carries at most 8 doubles, and a GMRES step sums up to restart + 1.  GMRES across ranks is an entry
 * of its own with a communicator of its own, rdc_solve_dist_gmres (below, behind rdc_solve_dist_mg). */
/* The last GMRES solve on this mesh: *restart = the restart length it ran with, *basis_bytes = device bytes of its basis
 * ((restart + 1) * n_owned * nvar * 8; behind rdc_solve_dist_gmres this rank's, whose slots have ghost tails: n_nodes for n_owned), *cycles = the cycles it began (restarts + 1; 0 if it needed no step).  Any pointer may be
 * NULL.  RDC_ERR_STATE before any GMRES solve on this mesh. */
int rdc_solve_gmres_stats(rdc_ctx* ctx, int32_t* restart, int64_t* basis_bytes, int32_t* cycles);
/* Test hook, read-only like rdc_solve_mg_apply: the Arnoldi process itself, which a converged solve cannot show (the true residual
 * at every restart repairs a process that is subtly wrong, at the price of iterations).  The call first does what a solve with
 * `precond` (mixed != 0: rdc_solve_mixed) does before its first iteration, then sets v_0 = d_v0 / ||d_v0|| and runs `steps` Arnoldi
 * steps, 1 <= steps <= "gmres_restart", with exactly the kernels and the host loop of a cycle; "gmres_refine" is honoured.
 * d_v0: DEVICE, n_owned*nvar doubles.  d_V: DEVICE, receives the *steps_done + 1 basis vectors, n_owned*nvar doubles each (room for
 * steps + 1).  H: HOST, (restart + 1) x restart doubles, column-major: the raw Hessenberg matrix before any rotation, zeros where no
 * entry was computed.  *steps_done < steps if h_{j+1,j} = 0 (that step counts; the last vector is then the zero remainder) or a
 * step was not finite (it does not count).  RDC_ERR_UNSUPPORTED on a context with ghost nodes; RDC_ERR_INVALID for a null pointer,
 * steps out of range, an unknown precond, or diagonal blocks that cannot be inverted (nothing is run).  Never modifies the CSR
 * values or the rhs; works whatever "solve_method" is.  Synchronises. */
int rdc_solve_gmres_arnoldi(rdc_ctx* ctx, int precond, int mixed, const double* d_v0, int steps, double* d_V, double* H,
                            int32_t* steps_done);

/* ---- partitioned solve (additive: RDC_ABI_VERSION stays 3): the BiCGStab of rdc_solve / rdc_solve_mixed across ranks, on
 * contexts with one ghost layer (n_owned < n_nodes; owned nodes first, ghosts behind them).  Every rank calls with its own
 * context; the ranks together solve the global system whose rows they own.  The library itself knows no MPI and no RCCL:
 * the communication comes in as three callbacks, which a torch.distributed harness and an MPI adapter can both supply
 * (INTEGRATION.md).
 *
 * What is exchanged: per iteration the ghost values of the two search directions p and s, one exchange
 * before each of the two operator applications; the ghost values of x before every true residual; and three all-reduces
 * per iteration of 2, 2 and 3 doubles (6 after the first true residual, 4 after every later one).  Every inner product, norm and
 * counter that decides anything is the all-reduced one, so reason, iterations, restarts, bad_blocks, matrix_bits and all
 * norms of rdc_solve_info are GLOBAL and identical on every rank, and every early return (bad diagonal, not finite, the
 * FP64 fall-back of a mixed solve, b = 0) is taken by all ranks together.
 *
 * Stream contract.  The callbacks run on the calling host thread, in program order.  `hip_stream` is the context's stream.
 * What the library enqueued on it before a callback produces that callback's inputs (d_send, the d_vals of an all-reduce):
 * the callee orders its transfer behind that work, by enqueueing on the same stream or by synchronising it.  When
 * exchange_end or allreduce_sum returns, the received values are ordered on `hip_stream` before anything enqueued later.
 * Between exchange_begin and exchange_end the library enqueues the operator over the rows that read no ghost value; nothing
 * it enqueues there reads d_recv or writes d_send.  allreduce_sum must deliver the same bits on every rank (RCCL and gloo
 * both do).  A callback returns 0, or non-zero to abort: rdc_solve_dist then returns RDC_ERR_COMM, calls no further
 * callback, and x holds the last iterate. */
typedef struct rdc_solve_comm {
  void* user;
  /* d_send: n_send*nvar doubles packed by the library in plan order; d_recv: the ghost tail of the vector being
     exchanged (n_ghost*nvar doubles, local ghost order).  The callee slices both per peer. */
  int (*exchange_begin)(void* user, const double* d_send, double* d_recv, void* hip_stream);
  int (*exchange_end)(void* user, void* hip_stream);
  int (*allreduce_sum)(void* user, double* d_vals, int32_t n, void* hip_stream);   /* in place, n <= 8 */
} rdc_solve_comm;

/* The send list of the uploaded mesh: send_nodes[i] = the owned local node whose nvar values are entry i of d_send
 * (a node may appear more than once: once per peer that has it as a ghost).  Copied; kept until the next mesh upload.
 * The option "interior_nodes" = n_int as it stands at this call (set it before the mesh upload, as for the two-part assembly)
 * makes every operator application overlap the exchange with the rows of the nodes [0, n_int); unset or 0: exchange first.
 * RDC_ERR_INVALID if a send id is not an owned node, if n_int > n_owned, or if a node below n_int has a ghost column. */
int rdc_solve_dist_plan(rdc_ctx* ctx, int64_t n_send, const int32_t* send_nodes);   /* owned local node ids, send order */
/* The contract of rdc_solve (mixed == 0) or rdc_solve_mixed (mixed != 0), across ranks.  d_x: DEVICE pointer, n_nodes*nvar
 * doubles in local numbering.  On entry the owned rows hold the initial guess, the ghost rows are ignored.  On exit the
 * owned rows hold the solution and the ghost rows the owners' values of it (the last true residual has just exchanged them),
 * whatever info->reason is; b = 0 gives x = 0 in 0 iterations, ghost rows included; RDC_SOLVE_BAD_DIAGONAL and a first
 * residual that is not finite leave the owned rows untouched.  precond: RDC_PRECOND_NONE, _JACOBI, _BLOCK_JACOBI, and with
 * mixed == 0 RDC_PRECOND_ILU0_LOCAL (above);
 * RDC_PRECOND_MULTIGRID gives RDC_ERR_UNSUPPORTED here (its coarse exchanges need sizes: rdc_solve_dist_mg below).  RDC_ERR_STATE on a context with
 * ghost nodes that has no plan.  A context without ghosts, with an empty or no plan and a communicator of world size 1 (an
 * exchange that does nothing, an all-reduce that leaves d_vals as they are) is legal and returns, bit for bit, what
 * rdc_solve / rdc_solve_mixed return.  Blocks the host until done.  Never modifies the CSR values or the rhs. */
int rdc_solve_dist(rdc_ctx* ctx, const rdc_solve_params* p, const rdc_solve_comm* comm, int mixed,
                   double* d_x, rdc_solve_info* info);

/* ---- multigrid across ranks (additive: RDC_ABI_VERSION stays 3): rdc_solve_dist with the V(1,1) cycle of RDC_PRECOND_MULTIGRID.
 * Aggregates never cross a partition: every rank aggregates the nodes it owns over the edges whose two ends it owns, so a
 * rank owns whole coarse rows and builds them without communication.  What every level needs is a ghost layer: the coarse
 * ghosts of a rank are the aggregates its peers made of its fine ghosts, learnt once per level by one exchange of aggregate
 * numbers (width 1, as doubles) when the hierarchy is built -- collectively, at the first such solve after a plan; a new plan
 * or mesh upload drops it.  Levels are added until the level has at most 40 nodes over all ranks, 10 levels exist or no rank
 * merged anything; every rank ends with the same number of levels, and with one rank the hierarchy is that of rdc_solve.
 * Inside a cycle every operator application exchanges its argument first: level 0 through exchange_begin / exchange_end with
 * the rows below "interior_nodes" in between, every level below through the sized pair, then one launch over the owned rows.
 * With L levels an iteration makes 6 exchanges of the plan's size and 2 (2 (L - 2) + 7) sized ones (L >= 2); the three
 * all-reduces per iteration are unchanged, since the cycle has no inner product. */
/* Per-peer segment lengths, in nodes, of the send list and of the ghost tail of the plan: peer k is the k-th peer of this call
 * (rank ids stay with the caller), the order is that of the send list and of the ghost tail, zeros are allowed.
 * RDC_ERR_STATE before rdc_solve_dist_plan; RDC_ERR_INVALID if a count is negative or the sums are not n_send and n_ghost. */
int rdc_solve_dist_plan_peers(rdc_ctx* ctx, int32_t n_peers, const int64_t* send_count, const int64_t* ghost_count);
/* The communicator of rdc_solve_dist and an exchange whose sizes come with the call, for the levels below the matrix.  d_send and
 * d_recv are as in exchange_begin; send_off and recv_off are HOST arrays of n_peers + 1 offsets in doubles: peer k gets
 * d_send[send_off[k] .. send_off[k + 1]) and delivers d_recv[recv_off[k] .. recv_off[k + 1]); an empty segment on one side is
 * empty on the peer's side too.  The callee only slices by what it is given.  The stream contract is that of exchange_begin /
 * exchange_end; nothing is enqueued between a sized begin and its end. */
typedef struct rdc_solve_comm_sized {
  rdc_solve_comm base;
  int (*exchange_sized_begin)(void* user, const double* d_send, double* d_recv, int32_t n_peers, const int64_t* send_off,
                              const int64_t* recv_off, void* hip_stream);
  int (*exchange_sized_end)(void* user, void* hip_stream);
} rdc_solve_comm_sized;
/* The contract of rdc_solve_dist with p->precond = RDC_PRECOND_MULTIGRID (or RDC_PRECOND_MULTIGRID_GS_LOCAL, above: the same
 * callbacks, other sweeps); any other preconditioner is RDC_ERR_INVALID.
 * RDC_ERR_STATE on a context with ghost nodes that lacks the plan or the peer counts.  A singular diagonal block on any level
 * of any rank gives RDC_SOLVE_BAD_DIAGONAL on every rank, x untouched.  A callback that returns non-zero (while the hierarchy
 * is built included) gives RDC_ERR_COMM and no further callback.  A context without ghosts and a communicator of world size
 * 1 returns, bit for bit, what rdc_solve / rdc_solve_mixed return with RDC_PRECOND_MULTIGRID.  rdc_solve_mg_levels and
 * rdc_solve_mg_stats then report this rank's levels: the nodes it owns and the node blocks of its rows. */
int rdc_solve_dist_mg(rdc_ctx* ctx, const rdc_solve_params* p, const rdc_solve_comm_sized* comm, int mixed,
                      double* d_x, rdc_solve_info* info);

/* ---- restarted GMRES(m) across ranks (additive: RDC_ABI_VERSION stays 3): the GMRES of rdc_solve / rdc_solve_mixed under
 * "solve_method" = 1, on the contexts, plans and preconditioners of rdc_solve_dist and rdc_solve_dist_mg.  With RDC_PRECOND_ILU0_LOCAL
 * this is what PETSc runs by default under mpirun: GMRES(30), one classical Gram-Schmidt pass, block Jacobi between the ranks,
 * ILU(0) inside each.  The entry runs GMRES whatever "solve_method" is (the option chooses for the entries that have no method in
 * their name) and honours "gmres_restart" and "gmres_refine".
 *
 * What is exchanged ("Across ranks").  Per Arnoldi step j: the ghost values of v_j (of M v_j with a right
 * preconditioner), one exchange of the plan's size before the operator application, received straight into the ghost tail of the
 * vector; one wide all-reduce of j + 2 doubles per Gram-Schmidt pass (h_0..j and (w, w) together; one pass, or two with
 * "gmres_refine" = 1) and one of 1 double for the norm of the remainder: 2 or 3 wide all-reduces per step.  Per cycle, and once at
 * the start: the ghost values of x and one allreduce_sum for the true residual (6 doubles the first time, 5 behind an update of x:
 * the fifth carries the count of entries that would not have been finite, 4 otherwise).  Without multigrid a solve of `iterations`
 * steps and `restarts` restarts therefore makes iterations + restarts + 2 exchanges, (2 or 3) * iterations wide all-reduces and
 * restarts + 2 calls of allreduce_sum.  With RDC_PRECOND_MULTIGRID every application of the cycle (one per step, one per update of
 * x) adds the exchanges of rdc_solve_dist_mg's cycle; the cycle has no inner product.  Dots and norms run over the owned rows only;
 * everything that decides -- the residual estimate, the flags of a step, y -- is computed from all-reduced values, so every rank
 * takes the same branch.
 *
 * The communicator.  `sized` is that of rdc_solve_dist_mg; its sized pair may be NULL unless p->precond == RDC_PRECOND_MULTIGRID.
 * allreduce_sum_wide sums d_vals[0 .. n) over the ranks in place, 1 <= n <= 128 + 2, under the stream contract of allreduce_sum: the
 * library has enqueued what produces d_vals on `hip_stream`, the sums are ordered on it when the callback returns, and every rank
 * gets the same bits.  An MPI adapter: MPI_Allreduce of n doubles. */
typedef struct rdc_solve_comm_wide {
  rdc_solve_comm_sized sized;   /* the sized pair may be NULL unless p->precond == RDC_PRECOND_MULTIGRID or RDC_PRECOND_MULTIGRID_GS_LOCAL */
  int (*allreduce_sum_wide)(void* user, double* d_vals, int32_t n, void* hip_stream);   /* in place, n <= 128 + 2 */
} rdc_solve_comm_wide;
/* The contract of rdc_solve_dist (mixed: of its mixed form), with GMRES(m) as the method.  precond: RDC_PRECOND_NONE, _JACOBI,
 * _BLOCK_JACOBI; RDC_PRECOND_ILU0_LOCAL (mixed != 0 only with "ilu_factor_bits" = 32, as in rdc_solve_dist); RDC_PRECOND_MULTIGRID
 * through the sized exchanges and the rank-local hierarchy of rdc_solve_dist_mg (RDC_ERR_STATE on a ghosted context without peer
 * counts, RDC_ERR_UNSUPPORTED under "mg_smoother" = 1).  RDC_PRECOND_ILU0 is RDC_ERR_UNSUPPORTED.  RDC_ERR_INVALID for a NULL
 * callback (the sized pair only if the multigrid is asked for); RDC_ERR_STATE on a context with ghost nodes and no plan.  Every
 * refusal comes before any callback and leaves x untouched.  Everything rdc_solve_dist promises carries over: rdc_solve_info is
 * global and identical on every rank, the ghost rows of x are filled on exit, b = 0 gives x = 0, RDC_SOLVE_BAD_DIAGONAL on every rank
 * leaves the owned rows untouched, a callback that returns non-zero gives RDC_ERR_COMM and no further callback, no NaN or inf is ever
 * written into x, residual_norm is the true FP64 residual.  iterations counts Arnoldi steps, restarts the cycles after the first;
 * rdc_solve_gmres_stats then reports this rank's basis.  A context without ghosts and a communicator of world size 1 returns, bit for
 * bit (info and x), what rdc_solve / rdc_solve_mixed return under "solve_method" = 1.  Blocks the host until done.  Never modifies
 * the CSR values or the rhs.  Not implemented across ranks: RDC_PRECOND_ILU0, "mg_smoother" = 1, a merged single-reduction
 * orthogonalisation. */
int rdc_solve_dist_gmres(rdc_ctx* ctx, const rdc_solve_params* p, const rdc_solve_comm_wide* comm, int mixed,
                         double* d_x, rdc_solve_info* info);
/* Test hook: the collective form of rdc_solve_gmres_arnoldi, on the communicator, plan and preconditioners of rdc_solve_dist_gmres.
 * Every rank passes its owned rows of v_0 (d_v0: DEVICE, n_owned*nvar doubles) and receives its owned rows of the basis (d_V: DEVICE,
 * *steps_done + 1 vectors of n_owned*nvar doubles, room for steps + 1); H (HOST, (restart + 1) x restart, column-major) and
 * *steps_done are identical on every rank.  Callbacks: one allreduce_sum (6 doubles: the counters of the set-up, so that all ranks
 * refuse singular blocks together), with RDC_PRECOND_MULTIGRID those that build the hierarchy, one wide all-reduce of 1 double for
 * ||v_0||, then per step what a step of rdc_solve_dist_gmres makes.  Refusals as rdc_solve_dist_gmres, and steps out of
 * 1 .. "gmres_restart" or bad diagonal blocks on any rank are RDC_ERR_INVALID on every rank.  Synchronises. */
int rdc_solve_dist_gmres_arnoldi(rdc_ctx* ctx, const rdc_solve_comm_wide* comm, int precond, int mixed, const double* d_v0, int steps,
                                 double* d_V, double* H, int32_t* steps_done);

/* ---- device-resident Newton solve of the solid system (additive, RDC_ABI_VERSION stays 3): what SolidSystem::solve() does
 * through libMesh's NewtonSolver (src/solid_system.C:84-100,380), as the host mirror states it (rdcfes_amd/host/rdc_host.h,
 * SolidSystem::solve), in one call that hands no matrix, rhs or vector back.  Single partition.
 * The unknowns are the context's CURRENT coordinates: the start iterate on entry, as rdc_mesh_upload, rdc_mesh_update_coords or
 * a device-side write left them, the result on exit.  Undeformed coordinates, fibre, materials and sides are those set in the
 * context; pseudo_time comes with rdc_solid_params, so the caller runs the load steps.  Per Newton iteration:
 *   1. rdc_solid_assemble (R and J), ||R||_2: RDC_NEWTON_CONVERGED_RESIDUAL if <= absolute_residual_tolerance or
 *      <= relative_residual_tolerance * first residual; RDC_NEWTON_MAX_ITS if max_nonlinear_iterations have been taken;
 *   2. J delta = -R from delta = 0 with rdc_solve (mixed: rdc_solve_mixed) and `linear`; RDC_SOLVE_MAX_ITS is used as it is;
 *   3. u = u0 + step * delta, step = 1; with require_reduction a residual-only assembly there, and step is halved while ||R(u)|| is
 *      not below ||R(u0)|| and step >= 1e-3 (u is always recomputed from the saved u0; a trial residual that is not finite halves);
 *   4. ||step * delta||_2 <= relative_step_tolerance * ||u||_2: one residual-only assembly for last_residual, RDC_NEWTON_CONVERGED_STEP.
 * A solver outcome is not an error status: the call returns RDC_OK and info->reason tells.  On return the CSR values and rhs are
 * those of the last assembly of the call (the rhs always at the returned coordinates, unless they were restored).
 * Refused before anything is launched: what rdc_solid_assemble refuses (nvar != 3: RDC_ERR_INVALID; undeformed coordinates, fibre
 * or materials unset: RDC_ERR_STATE); a context with ghost nodes (RDC_ERR_UNSUPPORTED); parameters out of range, tolerances that
 * are NaN, infinite or negative, an unknown precond (RDC_ERR_INVALID).  The linear solve refuses what rdc_solve / rdc_solve_mixed
 * refuse, with their status; the coordinates are then the start iterate.  Reads the linear-solve settings of rdc_set_option. */
typedef struct rdc_solid_newton_params {
  int32_t max_nonlinear_iterations;      /* "solver/nonlinear/max_nonlinear_iterations"; 1 .. 1000 */
  int32_t require_reduction;             /* "solver/nonlinear/require_reduction": halve the step while ||R|| does not go down */
  double  relative_step_tolerance, relative_residual_tolerance, absolute_residual_tolerance;
  rdc_solve_params linear;               /* rel_tol = "solver/linear/initial_linear_tolerance", max_its, precond; rhs_scale is ignored (the library uses -1) */
  int32_t mixed;                         /* 0: rdc_solve, 1: rdc_solve_mixed */
  int32_t reserved;
} rdc_solid_newton_params;

#define RDC_NEWTON_CONVERGED_RESIDUAL 0
#define RDC_NEWTON_CONVERGED_STEP     1
#define RDC_NEWTON_MAX_ITS            2
#define RDC_NEWTON_LINEAR_FAILED      3   /* BAD_DIAGONAL, BREAKDOWN or NOT_FINITE of the linear solve: coordinates = last accepted iterate */
#define RDC_NEWTON_NOT_FINITE         4   /* a residual norm was NaN/inf: coordinates = last iterate with a finite residual */

typedef struct rdc_solid_newton_info {
  int32_t reason, nonlinear_iterations, linear_iterations, assemblies, halvings, last_linear_reason;
  double  first_residual, last_residual, last_step_norm, last_solution_norm;
  float   device_ms; int32_t reserved;
} rdc_solid_newton_info;

int rdc_solid_newton(rdc_ctx* ctx, const rdc_solid_params* p, const rdc_solid_newton_params* np, rdc_solid_newton_info* info);
/* per Newton iteration of the last call on this context: ||R|| before the solve, accepted step length, linear iterations, linear
 * reason.  *n = the iterations the call took (one more if it ended with RDC_NEWTON_LINEAR_FAILED: that iteration is listed with
 * step 0); the first min(*n, cap) entries of every array that is not NULL are written. */
int rdc_solid_newton_history(rdc_ctx* ctx, int cap, double* residual, double* step, int32_t* lin_its, int32_t* lin_reason, int32_t* n);

/* ---- Newton solve of the solid system across ranks (additive: RDC_ABI_VERSION stays 3): the contract of rdc_solid_newton, across
 * the ranks of `comm`.  Every rank calls with its own context, which may have one ghost layer (owned nodes first, ghosts behind
 * them) and then carries the send list of rdc_solve_dist_plan (width nvar = 3: the coordinate array [node][3] is the dof layout).
 * Parameters, info and rdc_solid_newton_history are those of rdc_solid_newton.
 *
 * What is global.  Every norm newton's decisions read -- ||R||, ||step delta||, ||u|| -- is the norm over the owned rows of all
 * ranks, and rdc_solve_info of every linear solve is global, so every rank takes the same branch, and info and the history are
 * identical on every rank, except info->device_ms, which is this rank's own.
 *
 * What the entry itself communicates.  (1) On entry ONE exchange of the coordinates: the library packs the owned coordinates of the
 * plan's send nodes and calls exchange_begin / exchange_end with d_recv = the ghost tail of the coordinate array.  Ghost rows of the
 * coordinates are ignored on entry and hold the owners' values on exit: after this exchange every rank moves its ghost coordinates
 * itself, u = u0 + step * delta over ALL local nodes, from a delta whose ghost rows the partitioned linear entry returned holding
 * the owners' values -- rdc_solve_dist, rdc_solve_dist_mg and rdc_solve_dist_gmres return them so whatever info->reason is -- by the
 * same arithmetic on the same bits as the owner, so a ghost coordinate stays bit for bit its owner's through steps, halving trials
 * and the restore.  (2) Before each host read one allreduce_sum of n = 8 doubles, the whole 64-byte record of the loop (three sums
 * over the owned rows, five zeros): one behind each full assembly, each step or trial, and each measuring accept.  No linear entry
 * makes an all-reduce of that length.  Everything else is what the linear entry exchanges.
 *
 * The linear solve.  "solve_method" = 1: rdc_solve_dist_gmres; otherwise linear.precond RDC_PRECOND_MULTIGRID or
 * RDC_PRECOND_MULTIGRID_GS_LOCAL: rdc_solve_dist_mg; otherwise rdc_solve_dist; `mixed` is passed through.  Of `comm`,
 * exchange_begin, exchange_end and allreduce_sum are always required, the sized pair only for the two multigrid preconditioners,
 * allreduce_sum_wide only under "solve_method" = 1; the others may be NULL.  The linear entries keep their own refusals
 * (RDC_PRECOND_ILU0, "mg_smoother" = 1 under RDC_PRECOND_MULTIGRID, missing peer counts, ...): their status comes back from the first
 * solve, with the owned coordinates as on entry.
 *
 * Refused before any callback: what rdc_solid_newton refuses, except ghost nodes; RDC_ERR_STATE for a context with ghost nodes
 * and no send list; RDC_ERR_INVALID for a NULL communicator or a required callback that is NULL.  Every one of these depends only on
 * inputs that are the same on every rank (the mesh's nvar, what was set, the parameters, the options, the communicator's shape), so
 * they are collective by construction: either every rank refuses or none does.
 *
 * A rank that owns no node takes part in every callback with zero sums and does not return early.  If a callback, of the loop or of
 * a linear solve, returns non-zero the entry returns RDC_ERR_COMM, makes no further callback, and leaves the coordinates finite, as
 * the last executed action left them.  NOT collective, as for the other partitioned entries: HIP errors, and a failure of an assembly
 * in the middle of the loop; the other ranks then wait in their next callback, and ending them is the caller's business.
 * On a context without ghosts, with a communicator of world size 1, the entry launches and returns what rdc_solid_newton does. */
int rdc_solid_newton_dist(rdc_ctx* ctx, const rdc_solid_params* p, const rdc_solid_newton_params* np, const rdc_solve_comm_wide* comm,
                          rdc_solid_newton_info* info);

/* ---- post-solve nodal kernel: negativity clamp of check_solution,
 * src/pihna.C:785-790, applied in place to a device-resident field ---- */
int rdc_clamp_nonnegative(rdc_ctx* ctx, int field);

/* RIPF check_solution, src/ripf.C:675-775, on device-resident fields of a 3-variable context.  Per node:
 *   RDC_FIELD_OLD_SOLUTION  (the freshly solved state) is clamped in place: HU to [HU_min, HU_max], cc, fb >= 0 (:722-724);
 *   RDC_FIELD_TIME_DERIV    = (clamped - RDC_FIELD_PREV_SOLUTION) / time_step                          (:738-740);
 *   RDC_FIELD_RT_DOSE[2]    = total dose of the fractionation schedule on `day` from [0] broad, [1] focus (:754-758);
 *   RDC_FIELD_PREV_SOLUTION = the UNCLAMPED solved state, as upstream's `prev_soln = soln`             (:769);
 *   RDC_FIELD_AUX_NODAL     = {TIME_DERIV[1], TIME_DERIV[2], RT total}: what the next rdc_assemble_ripf reads (:470-478).
 * *rt_total_max receives max(-1, max over the context's nodes of RT total) (:705,761); upstream stores it truncated
 * to int in "RT_dose/total/max" and aborts when it is <= 0 (:771-772) -- with several ranks reduce it with MAX first.
 * TIME_DERIV, AUX_NODAL are (re)allocated as needed; OLD_SOLUTION, PREV_SOLUTION, RT_DOSE must have been set. */
typedef struct rdc_ripf_check_params {
  double time_step;              /* "time_step"                 */
  double HU_min, HU_max;         /* "HU/min", "HU/max"          */
  int32_t RT_broad_fractions;    /* "RT_dose/broad/fractions"   */
  int32_t RT_focus_fractions;    /* "RT_dose/focus/fractions"   */
  int32_t day;                   /* floor(system.time), :703    */
  int32_t _pad;
} rdc_ripf_check_params;
int rdc_ripf_check_solution(rdc_ctx* ctx, const rdc_ripf_check_params* p, double* rt_total_max);

/* SolidSystem::post_process, src/solid_system.C:394-538: per element the plain average over
 * the quadrature points of the Cauchy stress and of F*eta, then hydrostatic pressure (:522), von Mises stress (:524)
 * -- upstream takes both from the principal stresses of eigen_decomposition (src/eig3.C:261-271); they are the
 * invariants tr/3 and sqrt(I1^2 - 3 I2), which is what the kernel evaluates -- and the current fibre vector (:526).
 * Uses the mesh coordinates, RDC_FIELD_UNDEFORMED_XYZ, RDC_FIELD_ELEM_FIBRE and the materials of the context.
 * Host outputs (any may be NULL): pressure [n_elem], von_mises [n_elem], fibre_current [n_elem][3]. */
int rdc_solid_post_process(rdc_ctx* ctx, const rdc_solid_params* p, double* pressure, double* von_mises,
                           double* fibre_current);

/* save_solution of PIHNA, src/pihna.C:842-976 ("CSV volume integrals"): the four element-volume
 * sums of the CSV line -- an element counts when ALL its nodes have (c+h), n, v, (n+c+h+v)/cells_max_capacity inside
 * the closed range -- over the first n_elem elements of the context (pass the number of elements the rank owns, or
 * -1 for all; upstream loops over every active element on rank 0), read from RDC_FIELD_OLD_SOLUTION (5 unknowns).
 * out[4] = {ACTIVE_TUMOR_VOLUME, NECROTIC_VOLUME, VASCULARITY_VOLUME, TOTAL_CELL_VOLUME}; with several ranks add them. */
typedef struct rdc_pihna_ranges {
  double active_tumor_min, active_tumor_max;   /* "range/active_tumor/min,max" */
  double necrotic_min, necrotic_max;           /* "range/necrotic/min,max"     */
  double vascularity_min, vascularity_max;     /* "range/vascularity/min,max"  */
  double total_cell_min, total_cell_max;       /* "range/total_cell/min,max"   */
  double cells_max_capacity;                   /* "cells_max_capacity"         */
} rdc_pihna_ranges;
int rdc_pihna_volume_integrals(rdc_ctx* ctx, const rdc_pihna_ranges* r, int64_t n_elem, double* out4);

/* RIPF save_solution (replaces the element loop of src/ripf.C:812-858): out[2] = {Tumour_Volume, Fibrosis_Volume},
 * the volume of the elements ALL of whose nodes have HU inside [HU_min, HU_max] and cc (fb) >= min; read from
 * RDC_FIELD_OLD_SOLUTION (3 unknowns HU, cc, fb); first n_elem elements, -1 for all; with several ranks add. */
typedef struct rdc_ripf_ranges {
  double cc_HU_min, cc_HU_max, cc_min;   /* "range_cc/HU/min,max", "range_cc/min" */
  double fb_HU_min, fb_HU_max, fb_min;   /* "range_fb/HU/min,max", "range_fb/min" */
} rdc_ripf_ranges;
int rdc_ripf_volume_integrals(rdc_ctx* ctx, const rdc_ripf_ranges* r, int64_t n_elem, double* out2);

/* ADPM save_solution (replaces the element loop of src/adpm.C:747-813) over the brain parcellation = the set of
 * subdomain ids: elem_subdomain[n_elem] is elem->subdomain_id(), ids[n_ids] the parcellation (ascending, as the
 * std::set iterates).  out[n_ids][4] = {CONCENTRATION__A_b, CONCENTRATION__Tau, VOLUME__A_b, VOLUME__Tau}: the
 * volumes sum the elements of the region ALL of whose nodes lie inside the range (add over ranks); the
 * concentrations are -- as upstream, which assigns instead of accumulating (:780-783) -- the element average
 * sum_qp JxW*value / volume of the LAST element of the region in element order, and last_elem[n_ids] (may be
 * NULL) returns that element (-1: region empty here) so that several ranks can keep the one with the highest
 * global element.  Unknowns (PrP, A_b, Tau) from RDC_FIELD_OLD_SOLUTION (nvar = 3).  n_ids <= 2048. */
typedef struct rdc_adpm_ranges {
  double A_b_min, A_b_max;   /* "range/A_b/min,max" */
  double Tau_min, Tau_max;   /* "range/Tau/min,max" */
} rdc_adpm_ranges;
int rdc_adpm_parcellation_integrals(rdc_ctx* ctx, const rdc_adpm_ranges* r, const int32_t* elem_subdomain,
                                    const int32_t* ids, int32_t n_ids, int64_t n_elem, double* out,
                                    int64_t* last_elem);

/* ---- instrumentation ---- */
/* when enabled every rdc_assemble_* brackets its dominant kernel(s) -- the assembly kernel, or all
 * colour launches; not the small node-record pack -- with HIP events on the context stream */
int rdc_timing_enable(rdc_ctx* ctx, int on);
/* device time of the last assemble call in ms (valid after the stream has been synchronised) */
int rdc_timing_last_ms(rdc_ctx* ctx, float* ms);
/* sum of the device times of every assemble call since the last enable / sum, and their count;
 * synchronises on the recorded events and resets the pool (no host sync happens inside assemble) */
int rdc_timing_sum_ms(rdc_ctx* ctx, float* total_ms, int* n_calls);
/* the same, call by call (oldest first) into ms[0 .. min(*n_calls, capacity)): for the median / minimum of a timed run */
int rdc_timing_samples_ms(rdc_ctx* ctx, float* ms, int capacity, int* n_calls);

/* diagnostic only: call with host_out == NULL to arm (the next shipped-parameter PIHNA/TET4 assembly then
 * runs a separately compiled kernel that records s_memtime stamps per workgroup phase; *n_written = number
 * of values), call again with a buffer to fetch them: [workgroup][wave][6] shader-clock stamps.
 * With "kernel" = 7 and "ablate" = 4 set before arming, the stamped build is the element-visit kernel itself (results
 * unchanged): [cluster][wave][12] = 11 stamps + hardware id (tools/ev_timeline.py; "ev_resident" = 1: 6 stamps per cluster). */
int rdc_debug_stamps(rdc_ctx* ctx, long long* host_out, int64_t capacity, int64_t* n_written);

#ifdef __cplusplus
}
#endif
#endif /* RDC_ASSEMBLY_H */
