// g++ build of scaled_block_f32 (rdcfes_amd/csrc/rdc_solve.h) for tests/test_host_solve_f32.py: the block of the fp32
// copy of D^-1 A exactly as the set-up kernel of the mixed-precision solve computes it, callable from ctypes.
#include "../rdcfes_amd/csrc/rdc_solve.h"

extern "C" {

// out = fl32(dinv * a) for `count` consecutive nv x nv blocks (row-major); ok[i] = 1 if every entry of block i is finite in fp32
int shim_scaled_block_f32(int nv, long long count, const double* dinv, const double* a, float* out, int* ok) {
  for (long long i = 0; i < count; i++) {
    const long long o = i * nv * nv;
    if (nv == 3)
      ok[i] = rdc::scaled_block_f32<3>(*reinterpret_cast<const double (*)[3][3]>(dinv + o), *reinterpret_cast<const double (*)[3][3]>(a + o),
                                       *reinterpret_cast<float (*)[3][3]>(out + o)) ? 1 : 0;
    else if (nv == 5)
      ok[i] = rdc::scaled_block_f32<5>(*reinterpret_cast<const double (*)[5][5]>(dinv + o), *reinterpret_cast<const double (*)[5][5]>(a + o),
                                       *reinterpret_cast<float (*)[5][5]>(out + o)) ? 1 : 0;
    else
      return -1;
  }
  return 0;
}

// padded row stride of the fp32 copy, in floats
long long shim_f32_row_stride(int nv, long long blocks) { return rdc::f32_row_stride(nv, blocks); }

}
