// libmesh_adapter.C — the reference-side binding: drop-in replacements for the static
// assemble_<model>(EquationSystems&, const std::string&) callbacks of rdcFEs that forward to the
// C-ABI of librdc_assembly.so.
//
// NOT COMPILED IN THIS REPOSITORY'S BUILD: it needs libMesh (d3bda6c) and PETSc (746207a), neither of
// which exists in the build image.  It is written against the libMesh API the reference itself uses
// (src/pihna.C:318-395, :752-755).  What names no libMesh or PETSc type -- parameter key -> struct field, the solid system's
// material table and side list, the error path, schedule and pinning of the pipelined hand-back -- is include/rdc_marshal.h, which
// IS compiled and tested here (tests/test_host_marshal.py) and which the host mirror, rdcfes_amd/host/rdc_host.h, runs on the GPU.
// Left in this file, and so untested: bind(), the gathers through dof_number(), push_results(), push_results_device(),
// hand_back(), the MatSetValues consumer of the chunked hand-back, the residual / Jacobian insertion of SolidSystemGPU.  A failing
// C-ABI call or a missing parameter leaves a callback as an exception (std::runtime_error from marshal::check; libMesh's own).
//
// Usage in the reference tree:
//   1. add this file to src/ (Makefile:7 globs src/*.C), link with -lrdc_assembly;
//   2. in src/pihna.C replace   model.attach_assemble_function(assemble_pihna);          (:35)
//      by                       model.attach_assemble_function(rdc_gpu::assemble_pihna);
//      (same for src/ripf.C:27, src/coupled_hcc.C:37, src/adpm.C, src/proteas.C).  Nothing else changes:
//      libMesh still zeroes matrix/rhs, calls the callback once per time step on every rank, closes
//      matrix/rhs and hands them to PETSc KSP.
//   3. solid mechanics: replace   es.add_system<SolidSystem>("SolidSystem")           (src/solid.C:27, src/coupled_hcc.C:40)
//      by                         es.add_system<rdc_gpu::SolidSystemGPU>("SolidSystem")
//      -- a subclass of the reference's SolidSystem that overrides FEMSystem::assembly(), so that one
//      rdc_solid_assemble call replaces the per-element element_time_derivative / side_time_derivative
//      virtuals (src/solid_system.C:146-371) of every Newton iteration.
//   4. MORE THAN ONE MPI RANK: the GPU context of a rank holds its local elements PLUS the neighbouring elements that
//      touch one of its nodes, and reads the old solution (and the TD / RT / AUX / auxiliary systems) at all their
//      nodes.  libMesh's default algebraic ghosting (send_list) covers the dofs of local elements only, so before
//      es.init() call   rdc_gpu::add_ghost_layer(system)   for every system the callbacks read (the model system and,
//      where used, "RIPF-TimeDeriv", "RT", "AUX", "SolidSystem::auxiliary"): it attaches a PointNeighborCoupling with one
//      level to the system's DofMap, which puts those dofs into the ghosted vectors.  Without it sys.old_solution(dof)
//      on such a node is an out-of-range read in opt mode (an assert in dbg).  Serial runs need nothing.
//      The GPU of a rank is  node-local MPI rank % rdc_device_count()  (one rank per GPU).
#include "libmesh/boundary_info.h"
#include "libmesh/dof_map.h"
#include "libmesh/elem.h"
#include "libmesh/equation_systems.h"
#include "libmesh/mesh_base.h"
#include "libmesh/numeric_vector.h"
#include "libmesh/petsc_matrix.h"
#include "libmesh/point_neighbor_coupling.h"
#include "libmesh/transient_system.h"

#include "./solid_system.h"   // the reference's own header (src/solid_system.h): SolidSystemGPU derives from it

#include <map>
#include <unordered_map>
#include <vector>

#include "rdc_marshal.h"

using namespace libMesh;
namespace marshal = rdc::marshal;
using marshal::check;

namespace rdc_gpu {

// One GPU context per (rank, system): built on the first call, reused every time step.
struct Binding {
  rdc_ctx* ctx = nullptr;
  std::vector<dof_id_type> local_to_global_node;   // local node id -> libMesh node id (owned first, then ghosts)
  std::vector<dof_id_type> elem_ids;               // binding element -> libMesh element id (local elements + ghost layer)
  std::vector<PetscInt> row_ptr, col_glob;         // owned-row CSR with GLOBAL dof column ids
  std::vector<PetscInt> row_glob;                  // global dof id of owned row r = local node * nvar + var
  std::vector<double> val, rhs, u_old;
  dof_id_type n_owned = 0;
  marshal::PinState pins;                          // val / rhs registered with the HIP runtime once, for the async chunk copies
  bool pattern_frozen = false;                     // MAT_NEW_NONZERO_LOCATIONS switched off after the first assembly
  bool solid_bound = false;                        // SolidSystemGPU: materials and sides are in the context
};

static std::map<std::string, Binding> g_bindings;

// Unpin the hand-back arrays and destroy the GPU contexts: call it once the systems are done with (before MPI_Finalize /
// the end of main), or the arrays of the static map are freed at exit while still registered.  The next callback binds anew.
void release_bindings() {
  for (auto& kv : g_bindings) { kv.second.pins.release(kv.second.ctx); rdc_ctx_destroy(kv.second.ctx); }
  g_bindings.clear();
}

// N > 1 ranks: ghost the dofs of every element that shares a point with a local element (see the header, item 4).
// Call before es.init() for every system the GPU callbacks read.
void add_ghost_layer(System& sys) {
  static std::vector<std::unique_ptr<PointNeighborCoupling>> keep;   // the DofMap stores a reference
  keep.emplace_back(new PointNeighborCoupling());
  keep.back()->set_n_levels(1);
  sys.get_dof_map().add_algebraic_ghosting_functor(*keep.back());
}

// one rank per GPU: the device of this rank is its rank among the ranks of the same host
static int device_of_this_rank(const Parallel::Communicator& comm) {
  int ndev = 0;
  check(nullptr, rdc_device_count(&ndev), "rdc_device_count");
  if (ndev <= 0) libmesh_error_msg("no GPU visible to this rank");
  int local_rank = 0;
#ifdef LIBMESH_HAVE_MPI
  MPI_Comm node;
  MPI_Comm_split_type(comm.get(), MPI_COMM_TYPE_SHARED, (int)comm.rank(), MPI_INFO_NULL, &node);
  MPI_Comm_rank(node, &local_rank);
  MPI_Comm_free(&node);
#endif
  return local_rank % ndev;
}

// coordinates of the binding's nodes as the mesh holds them now, [local node][3]
static std::vector<double> node_coordinates(const MeshBase& mesh, const Binding& B) {
  std::vector<double> xyz(3 * B.local_to_global_node.size());
  for (size_t l = 0; l < B.local_to_global_node.size(); l++)
    for (int d = 0; d < 3; d++) xyz[3 * l + d] = mesh.node_ref(B.local_to_global_node[l])(d);
  return xyz;
}

// Marshal the rank's partition once: owned nodes first, then ghost nodes; elements = every active
// element touching an owned node (libMesh's active_local elements plus one ghost layer, which a
// DistributedMesh / ghosted ReplicatedMesh already holds).
static Binding& bind(EquationSystems& es, const std::string& name, unsigned int nvar) {
  Binding& B = g_bindings[name];
  if (B.ctx) return B;
  const MeshBase& mesh = es.get_mesh();
  const System& sys = es.get_system(name);
  const processor_id_type me = mesh.processor_id();
  std::unordered_map<dof_id_type, uint32_t> g2l;
  for (const auto& node : mesh.local_node_ptr_range()) { g2l[node->id()] = (uint32_t)B.local_to_global_node.size(); B.local_to_global_node.push_back(node->id()); }
  B.n_owned = (dof_id_type)B.local_to_global_node.size();
  std::vector<uint32_t> conn;
  std::vector<const Elem*> elems;
  for (const auto& elem : mesh.active_element_ptr_range()) {
    bool touches = false;
    for (unsigned int i = 0; i < elem->n_nodes(); i++) touches |= (elem->node_ref(i).processor_id() == me);
    if (touches) elems.push_back(elem);
  }
  const int nen = (int)elems.front()->n_nodes();   // TET4 (4) or HEX8 (8), one type per mesh
  for (const Elem* elem : elems) B.elem_ids.push_back(elem->id());
  for (const Elem* elem : elems)
    for (int i = 0; i < nen; i++) {
      const dof_id_type g = elem->node_id(i);
      auto it = g2l.find(g);
      if (it == g2l.end()) { it = g2l.emplace(g, (uint32_t)B.local_to_global_node.size()).first; B.local_to_global_node.push_back(g); }
      conn.push_back(it->second);
    }
  const std::vector<double> xyz = node_coordinates(mesh, B);
  check(nullptr, rdc_ctx_create(device_of_this_rank(mesh.comm()), &B.ctx), "rdc_ctx_create");
  check(B.ctx, rdc_mesh_upload(B.ctx, nen, (int64_t)elems.size(), (int64_t)B.local_to_global_node.size(), B.n_owned, conn.data(),
                               xyz.data(), (int)nvar), "rdc_mesh_upload");
  // pattern with LOCAL column ids -> global PETSc dof ids (dof_number(sys, var, 0))
  int64_t n_rows = 0, nnz = 0;
  check(B.ctx, rdc_csr_dims(B.ctx, &n_rows, &nnz), "rdc_csr_dims");
  std::vector<int64_t> rp(n_rows + 1);
  std::vector<int32_t> cl(nnz);
  check(B.ctx, rdc_csr_pattern_download(B.ctx, rp.data(), cl.data()), "rdc_csr_pattern_download");
  B.row_ptr.assign(rp.begin(), rp.end());
  B.col_glob.resize(nnz);
  for (int64_t k = 0; k < nnz; k++) {
    const Node& nd = mesh.node_ref(B.local_to_global_node[cl[k] / nvar]);
    B.col_glob[k] = (PetscInt)nd.dof_number(sys.number(), cl[k] % nvar, 0);
  }
  B.val.resize(nnz); B.rhs.resize(n_rows); B.u_old.resize(nvar * B.local_to_global_node.size());
  B.row_glob.resize(n_rows);
  for (int64_t r = 0; r < n_rows; r++)
    B.row_glob[r] = (PetscInt)mesh.node_ref(B.local_to_global_node[r / nvar]).dof_number(sys.number(), r % nvar, 0);
  return B;
}

// old_local_solution (ghosted) -> [local node][var], the layout of RDC_FIELD_OLD_SOLUTION, and into the context
static void upload_old_solution(const EquationSystems& es, const TransientLinearImplicitSystem& sys, Binding& B, unsigned int nvar) {
  const MeshBase& mesh = es.get_mesh();
  for (size_t l = 0; l < B.local_to_global_node.size(); l++) {
    const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
    for (unsigned int v = 0; v < nvar; v++) B.u_old[l * nvar + v] = sys.old_solution(nd.dof_number(sys.number(), v, 0));   // src/pihna.C:433
  }
  check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_OLD_SOLUTION, B.u_old.data(), (int64_t)B.u_old.size()), "rdc_field_upload");
}

// assembled owned rows -> system.matrix / system.rhs (what add_matrix / add_vector did, src/pihna.C:754-755)
static void push_results(const EquationSystems& es, TransientLinearImplicitSystem& sys, Binding& B, unsigned int nvar) {
  check(B.ctx, rdc_csr_download(B.ctx, B.val.data(), B.rhs.data()), "rdc_csr_download");
  Mat A = cast_ref<PetscMatrix<Number>&>(*sys.matrix).mat();
  const MeshBase& mesh = es.get_mesh();
  for (dof_id_type l = 0; l < B.n_owned; l++) {
    const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
    for (unsigned int a = 0; a < nvar; a++) {
      const PetscInt row = (PetscInt)nd.dof_number(sys.number(), a, 0);
      const PetscInt r = (PetscInt)(l * nvar + a), b = B.row_ptr[r], n = B.row_ptr[r + 1] - b;
      MatSetValues(A, 1, &row, n, &B.col_glob[b], &B.val[b], INSERT_VALUES);   // complete rows: no off-rank stash traffic
      sys.rhs->set(row, B.rhs[r]);
    }
  }
}

// The same hand-back, pipelined ("rdc/handback_chunks" > 1): marshal::hand_back_chunked cuts the owned node range into chunks,
// keeps two chunk downloads in flight on the context's copy stream and calls the consumer below for every chunk while the next
// travels; B.pins keeps val / rhs registered from the first call on.  The nvar rows of a node share one column set and lie back to
// back in the CSR array, so they are ONE dense nvar x ncols block for MatSetValues: one call per node block instead of one per row
// (rows of different nodes have different column sets: a chunk as a whole is not a dense block, so it cannot be a single call).
// After the first assembly the pattern is frozen (MAT_NEW_NONZERO_LOCATIONS off): PETSc then skips the search for new
// locations and any pattern drift is an error instead of a silent reallocation.
static void push_results_chunked(const EquationSystems& es, TransientLinearImplicitSystem& sys, Binding& B, unsigned int nvar, int n_chunks) {
  Mat A = cast_ref<PetscMatrix<Number>&>(*sys.matrix).mat();
  const MeshBase& mesh = es.get_mesh();
  std::vector<PetscInt> rows(nvar);
  marshal::hand_back_chunked(B.ctx, (int64_t)B.n_owned, n_chunks, B.val.data(), B.val.size(), B.rhs.data(), B.rhs.size(), B.pins, [&](int64_t n0, int64_t n1) {
    for (int64_t l = n0; l < n1; l++) {
      const Node& nd = mesh.node_ref(B.local_to_global_node[(size_t)l]);
      for (unsigned int a = 0; a < nvar; a++) rows[a] = (PetscInt)nd.dof_number(sys.number(), a, 0);
      const PetscInt b = B.row_ptr[(size_t)(l * nvar)], n = B.row_ptr[(size_t)(l * nvar) + 1] - b;
      // rows l*nvar .. l*nvar + nvar - 1: the same n columns (B.col_glob[b ..]), values row after row from B.val[b]
      MatSetValues(A, (PetscInt)nvar, rows.data(), n, &B.col_glob[(size_t)b], &B.val[(size_t)b], INSERT_VALUES);
      for (unsigned int a = 0; a < nvar; a++) sys.rhs->set(rows[a], B.rhs[(size_t)(l * nvar + a)]);
    }
  });
  if (!B.pattern_frozen) {   // takes effect for the NEXT assembly (this one may still have created locations)
    MatSetOption(A, MAT_NEW_NONZERO_LOCATIONS, PETSC_FALSE);
    B.pattern_frozen = true;
  }
}

#if defined(PETSC_HAVE_HIP) && defined(RDC_ADAPTER_DEVICE_HANDOFF)
// Device-pointer hand-off: with one rank and a MATSEQAIJHIPSPARSE system matrix PETSc's CSR value
// array IS the context's (same row order, columns ascending within a row -- rdc_csr_pattern_download is what the adapter
// preallocated from), so the hand-back is one device-to-device copy and the 5 GB never cross PCIe.  With several ranks PETSc
// keeps the diagonal and the off-diagonal block of MPIAIJ separately; the chunked host path above stays the portable one.
#include <hip/hip_runtime_api.h>
static bool push_results_device(TransientLinearImplicitSystem& sys, Binding& B) {
  Mat A = cast_ref<PetscMatrix<Number>&>(*sys.matrix).mat();
  PetscBool is_seq_hip = PETSC_FALSE;
  PetscObjectTypeCompare((PetscObject)A, MATSEQAIJHIPSPARSE, &is_seq_hip);
  if (!is_seq_hip) return false;
  double *d_val = nullptr, *d_rhs = nullptr;
  // d_val is only read here (the copy below): a binding that keeps it that way may set rdc_set_option(ctx, "const_rows", 2) once,
  // so that this hand-out does not stop the element-visit launches from leaving the a rows they find
  check(B.ctx, rdc_csr_values_device_ptr(B.ctx, &d_val, &d_rhs), "rdc_csr_values_device_ptr");
  PetscScalar* a = nullptr;
  MatSeqAIJHIPSPARSEGetArrayWrite(A, &a);                 // device pointer of the CSR values, write access
  check(B.ctx, rdc_synchronize(B.ctx), "rdc_synchronize");
  if (hipMemcpy(a, d_val, B.val.size() * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess) libmesh_error_msg("device hand-off copy failed");
  MatSeqAIJHIPSPARSERestoreArrayWrite(A, &a);
  // the rhs is small (nvar doubles per node): through the host as before
  check(B.ctx, rdc_csr_download(B.ctx, nullptr, B.rhs.data()), "rdc_csr_download");
  for (size_t r = 0; r < B.rhs.size(); r++) sys.rhs->set(B.row_glob[r], B.rhs[r]);
  return true;
}
#endif

// what every assemble_<model> callback does with the finished rows
static void hand_back(const EquationSystems& es, TransientLinearImplicitSystem& sys, Binding& B, unsigned int nvar) {
#if defined(PETSC_HAVE_HIP) && defined(RDC_ADAPTER_DEVICE_HANDOFF)
  if (B.pattern_frozen && push_results_device(sys, B)) return;   // from the second assembly on (the first one creates the pattern on the host path)
#endif
  const int chunks = es.parameters.have_parameter<int>("rdc/handback_chunks") ? es.parameters.get<int>("rdc/handback_chunks") : 8;
  if (chunks > 1) push_results_chunked(es, sys, B, nvar, chunks);
  else push_results(es, sys, B, nvar);
}

void assemble_pihna(EquationSystems& es, const std::string& system_name) {
  TransientLinearImplicitSystem& system = es.get_system<TransientLinearImplicitSystem>(system_name);
  libmesh_assert_equal_to(system.n_vars(), 5);
  Binding& B = bind(es, system_name, 5);
  const rdc_pihna_params p = marshal::read<rdc_pihna_params>(es.parameters);   // the keys assemble_pihna reads, src/pihna.C:358-381
  upload_old_solution(es, system, B, 5);
  check(B.ctx, rdc_assemble_pihna(B.ctx, &p), "rdc_assemble_pihna");
  hand_back(es, system, B, 5);
}

// src/coupled_hcc.C:414-649.  The mesh is the CURRENT configuration (SolidSystem::update moved the nodes,
// src/coupled_hcc.C:98-114), so the coordinates are refreshed before every assembly.
void assemble_hcc(EquationSystems& es, const std::string& system_name) {
  TransientLinearImplicitSystem& system = es.get_system<TransientLinearImplicitSystem>(system_name);
  libmesh_assert_equal_to(system.n_vars(), 3);
  Binding& B = bind(es, system_name, 3);
  const rdc_hcc_params p = marshal::read<rdc_hcc_params>(es.parameters);   // src/coupled_hcc.C:450-461
  check(B.ctx, rdc_mesh_update_coords(B.ctx, node_coordinates(es.get_mesh(), B).data()), "rdc_mesh_update_coords");
  upload_old_solution(es, system, B, 3);
  check(B.ctx, rdc_assemble_hcc(B.ctx, &p), "rdc_assemble_hcc");
  hand_back(es, system, B, 3);
}

// current_local_solution of any nodal system at the binding's nodes -> [local node][first..first+n) per node
static void gather_nodal(const EquationSystems& es, const System& sys, const Binding& B, unsigned int first_var, unsigned int n,
                         unsigned int stride, unsigned int offset, std::vector<double>& out) {
  const MeshBase& mesh = es.get_mesh();
  for (size_t l = 0; l < B.local_to_global_node.size(); l++) {
    const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
    for (unsigned int v = 0; v < n; v++) out[l * stride + offset + v] = sys.current_solution(nd.dof_number(sys.number(), first_var + v, 0));
  }
}

// src/ripf.C:337-673: additionally reads TD vars 1, 2 (src/ripf.C:470-471) and RT var 2 (:477-478)
void assemble_ripf(EquationSystems& es, const std::string& system_name) {
  TransientLinearImplicitSystem& system = es.get_system<TransientLinearImplicitSystem>(system_name);
  libmesh_assert_equal_to(system.n_vars(), 3);
  const System& TD = es.get_system<System>("RIPF-TimeDeriv");
  const System& RT = es.get_system<ExplicitSystem>("RT");
  Binding& B = bind(es, system_name, 3);
  const rdc_ripf_params p = marshal::read<rdc_ripf_params>(es.parameters);   // src/ripf.C:377-408
  std::vector<double> aux(3 * B.local_to_global_node.size());
  gather_nodal(es, TD, B, 1, 2, 3, 0, aux);   // cc, fb time derivatives -> aux[.][0], aux[.][1]
  gather_nodal(es, RT, B, 2, 1, 3, 2, aux);   // total dose -> aux[.][2]
  upload_old_solution(es, system, B, 3);
  check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_AUX_NODAL, aux.data(), (int64_t)aux.size()), "rdc_field_upload(aux)");
  check(B.ctx, rdc_assemble_ripf(B.ctx, &p), "rdc_assemble_ripf");
  hand_back(es, system, B, 3);
}

// src/adpm.C:324-652: unknowns PrP, A_b, Tau; the elemental "Tracts" system (3 CONSTANT MONOMIAL variables, :448-453)
// becomes RDC_FIELD_ELEM_TRACTS; decay/PrP is scaled with system.time (:367-413)
void assemble_adpm(EquationSystems& es, const std::string& system_name) {
  TransientLinearImplicitSystem& system = es.get_system<TransientLinearImplicitSystem>(system_name);
  libmesh_assert_equal_to(system.n_vars(), 3);
  const System& tracts = es.get_system<System>("Tracts");
  Binding& B = bind(es, system_name, 3);
  const rdc_adpm_params p = marshal::read_adpm(es.parameters, system.time);   // the angles are radians already in es.parameters (src/adpm.C:193)
  // per-element tract vectors in the binding's element order
  const MeshBase& mesh = es.get_mesh();
  std::vector<double> tr(3 * B.elem_ids.size());
  for (size_t e = 0; e < B.elem_ids.size(); e++) {
    const Elem& elem = mesh.elem_ref(B.elem_ids[e]);
    for (unsigned int d = 0; d < 3; d++) tr[3 * e + d] = tracts.current_solution(elem.dof_number(tracts.number(), d, 0));
  }
  upload_old_solution(es, system, B, 3);
  check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_ELEM_TRACTS, tr.data(), (int64_t)tr.size()), "rdc_field_upload(tracts)");
  check(B.ctx, rdc_assemble_adpm(B.ctx, &p), "rdc_assemble_adpm");
  hand_back(es, system, B, 3);
}

// src/proteas.C:338-705: unknowns hos, tum, nec, vsc, oed; the nodal "AUX" system {HU, RTD} -> RDC_FIELD_AUX_NODAL
// (only variable 0 is read by the assembly, at local node 1 of every element: src/proteas.C:472,481)
void assemble_proteas_model(EquationSystems& es, const std::string& system_name) {
  TransientLinearImplicitSystem& system = es.get_system<TransientLinearImplicitSystem>(system_name);
  libmesh_assert_equal_to(system.n_vars(), 5);
  const System& AUX = es.get_system<System>("AUX");
  Binding& B = bind(es, system_name, 5);
  const rdc_proteas_params p = marshal::read<rdc_proteas_params>(es.parameters);   // src/proteas.C:376-409
  std::vector<double> aux(3 * B.local_to_global_node.size(), 0.0);
  gather_nodal(es, AUX, B, 0, 2, 3, 0, aux);
  upload_old_solution(es, system, B, 5);
  check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_AUX_NODAL, aux.data(), (int64_t)aux.size()), "rdc_field_upload(aux)");
  check(B.ctx, rdc_assemble_proteas(B.ctx, &p), "rdc_assemble_proteas");
  hand_back(es, system, B, 5);
}

// ---- SolidSystem: FEMSystem::assembly() replaced wholesale -------------------------------------------------------
// libMesh's FEMSystem::assembly(get_residual, get_jacobian, ...) zeroes rhs / matrix, loops over the local elements
// (and their boundary sides) calling the reference's element_time_derivative / side_time_derivative virtuals
// (src/solid_system.C:146-371) and adds each element's residual and Jacobian into the global ones.  Here the loop is
// ONE GPU call on data marshalled from exactly what those virtuals read.  NewtonSolver, the PETSc linear solve,
// SolidSystem::update() (moves the mesh), run_solver / post_process / update_data stay the reference's code.
class SolidSystemGPU : public SolidSystem {
 public:
  SolidSystemGPU(EquationSystems& es, std::string name, unsigned int number) : SolidSystem(es, name, number) {}

  // Opt-in: solve() makes ONE call, rdc_solid_newton, in place of NewtonSolver + PETSc: the Newton iteration of
  // "solver/nonlinear/*" with the device-resident linear solve, and only the positions come back (no matrix, no rhs).
  // Single partition.  The linear solver is the context's (rdc_set_option "solve_method", "mg_smoother", ...) with the
  // preconditioner named here, "solver/linear/initial_linear_tolerance" and "solver/linear/max_linear_iterations".
  bool solve_on_device = false;
  int device_precond = RDC_PRECOND_BLOCK_JACOBI;
  bool device_mixed = false;
  rdc_solid_newton_info last_device = rdc_solid_newton_info();   // what that call reported

  virtual void solve() override {
    if (!solve_on_device) { SolidSystem::solve(); return; }
    EquationSystems& es = this->get_equation_systems();
    const MeshBase& mesh = es.get_mesh();
    if (mesh.n_processors() > 1) throw std::runtime_error("SolidSystemGPU::solve_on_device: single partition only");
    Binding& B = bind(es, this->name(), 3);
    const rdc_solid_params p = upload_iterate(es, mesh, B);
    rdc_solid_newton_params np = rdc_solid_newton_params();
    np.max_nonlinear_iterations = es.parameters.get<int>("solver/nonlinear/max_nonlinear_iterations");
    np.require_reduction = es.parameters.get<bool>("solver/nonlinear/require_reduction") ? 1 : 0;
    np.relative_step_tolerance = es.parameters.get<Real>("solver/nonlinear/relative_step_tolerance");
    np.relative_residual_tolerance = es.parameters.get<Real>("solver/nonlinear/relative_residual_tolerance");
    np.absolute_residual_tolerance = es.parameters.get<Real>("solver/nonlinear/absolute_residual_tolerance");
    np.linear.rel_tol = es.parameters.get<Real>("solver/linear/initial_linear_tolerance");
    np.linear.abs_tol = 0.0;
    np.linear.rhs_scale = -1.0;
    np.linear.max_its = es.parameters.get<int>("solver/linear/max_linear_iterations");
    np.linear.precond = device_precond;
    np.mixed = device_mixed ? 1 : 0;
    check(B.ctx, rdc_solid_newton(B.ctx, &p, &np, &last_device), "rdc_solid_newton");
    // the positions: the coordinate array has the layout of a 3-variable nodal field, so the slot of the old solution, which the
    // solid system does not use, is bound to it and downloaded as a field
    const size_t nn = B.local_to_global_node.size();
    std::vector<double> x(3 * nn);
    double* d_xyz = nullptr;
    check(B.ctx, rdc_mesh_coords_device_ptr(B.ctx, &d_xyz), "rdc_mesh_coords_device_ptr");
    check(B.ctx, rdc_field_bind_device(B.ctx, RDC_FIELD_OLD_SOLUTION, d_xyz, (int64_t)x.size()), "rdc_field_bind_device");
    check(B.ctx, rdc_field_download(B.ctx, RDC_FIELD_OLD_SOLUTION, x.data(), (int64_t)x.size()), "rdc_field_download(positions)");
    for (dof_id_type l = 0; l < B.n_owned; l++) {
      const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
      for (unsigned int d = 0; d < 3; d++) this->solution->set(nd.dof_number(this->number(), this->var[d], 0), x[3 * l + d]);
    }
    this->solution->close();
    this->update();   // SolidSystem::update(): current_local_solution, the mesh, "SolidSystem::displacement"
  }

  virtual void assembly(bool get_residual, bool get_jacobian, bool /*apply_heterogeneous_constraints*/ = false,
                        bool /*apply_no_constraints*/ = false) override {
    EquationSystems& es = this->get_equation_systems();
    const MeshBase& mesh = es.get_mesh();
    Binding& B = bind(es, this->name(), 3);
    const rdc_solid_params p = upload_iterate(es, mesh, B);
    check(B.ctx, rdc_solid_assemble(B.ctx, &p, get_jacobian ? 1 : 0), "rdc_solid_assemble");
    check(B.ctx, rdc_csr_download(B.ctx, get_jacobian ? B.val.data() : nullptr, B.rhs.data()), "rdc_csr_download");
    // owned rows -> system.matrix / system.rhs (FEMSystem::assembly zeroes them first; complete rows: no stash traffic)
    if (get_residual) this->rhs->zero();
    if (get_jacobian) this->matrix->zero();
    Mat A = get_jacobian ? cast_ref<PetscMatrix<Number>&>(*this->matrix).mat() : nullptr;
    for (dof_id_type l = 0; l < B.n_owned; l++) {
      const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
      for (unsigned int a = 0; a < 3; a++) {
        const PetscInt row = (PetscInt)nd.dof_number(this->number(), this->var[a], 0);
        const PetscInt r = (PetscInt)(l * 3 + a), b = B.row_ptr[r], n = B.row_ptr[r + 1] - b;
        if (get_jacobian) MatSetValues(A, 1, &row, n, &B.col_glob[b], &B.val[b], INSERT_VALUES);
        if (get_residual) this->rhs->set(row, B.rhs[r]);
      }
    }
    if (get_residual) this->rhs->close();
    if (get_jacobian) this->matrix->close();
  }

 private:
  // what assembly() and the device solve put into the context: once the materials and sides, every time the current iterate,
  // the undeformed positions and the reference fibre; returns the parameters of the call
  rdc_solid_params upload_iterate(EquationSystems& es, const MeshBase& mesh, Binding& B) {
    const System& aux = es.get_system<System>("SolidSystem::auxiliary");
    const System& fibre = es.get_system<System>("SolidSystem::fibre");
    const size_t nn = B.local_to_global_node.size(), ne = B.elem_ids.size();
    if (!B.solid_bound) {   // what does not change between Newton iterations
      // subdomain -> material table ("material/<id>/...", src/solid_system.C:183-190)
      const marshal::MaterialTable mt = marshal::material_table(es.parameters, (int64_t)ne, [&](int64_t e) { return mesh.elem_ref(B.elem_ids[(size_t)e]).subdomain_id(); });
      check(B.ctx, rdc_solid_set_materials(B.ctx, mt.elem_material.data(), (int32_t)mt.table.size(), mt.table.data()), "rdc_solid_set_materials");
      // boundary sides whose id is in "BCs" (src/solid_system.C:294-306) of EVERY element of the binding, ghost layer
      // included: the library adds a side's penalty terms only into rows of nodes this rank owns, so each rank ends up
      // with the complete rows of its nodes (a side next to the partition boundary is listed on both ranks)
      const marshal::SideList sl = marshal::side_list<Point>(es.parameters, [&](int bc, auto&& emit) {
        for (size_t e = 0; e < ne; e++) {
          const Elem& elem = mesh.elem_ref(B.elem_ids[e]);
          for (auto s : elem.side_index_range())
            if (mesh.get_boundary_info().has_boundary_id(&elem, s, cast_int<boundary_id_type>(bc))) emit((int64_t)e, (int32_t)s);
        }
      });
      check(B.ctx, rdc_solid_set_sides(B.ctx, (int64_t)sl.elem.size(), sl.elem.data(), sl.side.data(), sl.displacement.data()), "rdc_solid_set_sides");
      B.solid_bound = true;
    }
    // current node positions = the unknowns of the current Newton iterate (FEMContext::pre_fe_reinit moves the element's
    // nodes there); undeformed positions; reference fibre
    std::vector<double> x(3 * nn), X(3 * nn), eta(3 * ne);
    for (size_t l = 0; l < nn; l++) {
      const Node& nd = mesh.node_ref(B.local_to_global_node[l]);
      for (unsigned int d = 0; d < 3; d++) {
        x[3 * l + d] = this->current_solution(nd.dof_number(this->number(), this->var[d], 0));
        X[3 * l + d] = aux.current_solution(nd.dof_number(aux.number(), this->undefo_var[d], 0));   // :221-229
      }
    }
    for (size_t e = 0; e < ne; e++) {
      const Elem& elem = mesh.elem_ref(B.elem_ids[e]);
      for (unsigned int d = 0; d < 3; d++) eta[3 * e + d] = fibre.current_solution(elem.dof_number(fibre.number(), d, 0));   // :204-216
    }
    check(B.ctx, rdc_mesh_update_coords(B.ctx, x.data()), "rdc_mesh_update_coords");
    check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_UNDEFORMED_XYZ, X.data(), (int64_t)X.size()), "rdc_field_upload(undeformed)");
    check(B.ctx, rdc_field_upload(B.ctx, RDC_FIELD_ELEM_FIBRE, eta.data(), (int64_t)eta.size()), "rdc_field_upload(fibre)");
    return marshal::solid_params(es.parameters);
  }
};

}  // namespace rdc_gpu
