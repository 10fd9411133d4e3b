// g++ build of rdcfes_amd/csrc/rdc_solve.h for tests/test_host_solve.py: the block inverse and the index arithmetic the
// solver kernels use, callable from ctypes.
#include "../rdcfes_amd/csrc/rdc_solve.h"

extern "C" {

// in-place inverse of an nv x nv block (row-major); 1 = inverted, 0 = reported as singular / non-finite
int shim_block_inverse(int nv, double* m) {
  if (nv == 3) return rdc::block_inverse<3>(*reinterpret_cast<double (*)[3][3]>(m)) ? 1 : 0;
  if (nv == 5) return rdc::block_inverse<5>(*reinterpret_cast<double (*)[5][5]>(m)) ? 1 : 0;
  return -1;
}

int shim_precond_block(int nv, double* m, int precond) {
  if (nv == 3) return rdc::precond_block<3>(*reinterpret_cast<double (*)[3][3]>(m), precond) ? 1 : 0;
  if (nv == 5) return rdc::precond_block<5>(*reinterpret_cast<double (*)[5][5]>(m), precond) ? 1 : 0;
  return -1;
}

// col[csr_value_offset(node, a, k, b)] = csr_value_column(node, k, b) for every entry; returns the number of entries
// written, or -1 if an offset falls outside [0, nnz) or is written twice (col must come in filled with -1)
int64_t shim_expand_pattern(int nvar, int64_t n_owned, const int64_t* bptr, const int32_t* bcol, int64_t nnz, int32_t* col) {
  int64_t written = 0;
  for (int64_t n = 0; n < n_owned; n++)
    for (int a = 0; a < nvar; a++)
      for (int64_t k = 0; k < bptr[n + 1] - bptr[n]; k++)
        for (int b = 0; b < nvar; b++) {
          const int64_t o = rdc::csr_value_offset(bptr, nvar, n, a, k, b);
          if (o < 0 || o >= nnz || col[o] != -1) return -1;
          col[o] = (int32_t)rdc::csr_value_column(bptr, bcol, nvar, n, k, b);
          written++;
        }
  return written;
}

void shim_diag_blocks(int64_t n_owned, const int64_t* bptr, const int32_t* bcol, int64_t* out) {
  for (int64_t n = 0; n < n_owned; n++) out[n] = rdc::csr_diag_block(bptr, bcol, n);
}

}
