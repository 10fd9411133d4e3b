// A fake of the five C-ABI calls that rdc::marshal::hand_back_chunked and PinState make (include/rdc_marshal.h), for
// tests/host_marshal_main.cpp: no device, no library.  Every call is printed in order; rdc_csr_download_rows_async copies the
// rows of its node range from the source arrays given to fake_ctx_new at the call, as if the copy had already arrived.
#include <cstdio>
#include <cstring>
#include <string>

#include "../include/rdc_assembly.h"

struct rdc_ctx {
  int nvar;
  const int64_t* row_ptr;        // scalar rows, nvar per node
  const double *val, *rhs;       // what the "device" holds
  int next_ticket = 0;
  std::string fail_call, error;  // fake_fail: the next call of that name fails
};

static int status(rdc_ctx* c, const char* call) {
  if (c->fail_call != call) return RDC_OK;
  c->fail_call.clear();
  c->error = std::string("fake failure of ") + call;
  return RDC_ERR_INVALID;
}

extern "C" {
rdc_ctx* fake_ctx_new(int nvar, const int64_t* row_ptr, const double* val, const double* rhs) { return new rdc_ctx{nvar, row_ptr, val, rhs}; }
void fake_ctx_delete(rdc_ctx* c) { delete c; }
void fake_fail(rdc_ctx* c, const char* call) { c->fail_call = call; }

const char* rdc_last_error(const rdc_ctx* c) { return c ? c->error.c_str() : "no context"; }
int rdc_host_pin(rdc_ctx* c, void* p, size_t bytes) {
  std::printf("pin %p %zu\n", p, bytes);
  return status(c, "rdc_host_pin");
}
int rdc_host_unpin(rdc_ctx* c, void* p) {
  std::printf("unpin %p\n", p);
  return status(c, "rdc_host_unpin");
}
int rdc_csr_download_rows_async(rdc_ctx* c, int64_t n0, int64_t n1, double* val, double* rhs, int* ticket) {
  *ticket = c->next_ticket;
  c->next_ticket = (c->next_ticket + 1) % 16;
  std::printf("async %lld %lld %d\n", (long long)n0, (long long)n1, *ticket);
  const int64_t r0 = n0 * c->nvar, r1 = n1 * c->nvar;
  std::memcpy(val + c->row_ptr[r0], c->val + c->row_ptr[r0], (size_t)(c->row_ptr[r1] - c->row_ptr[r0]) * sizeof(double));
  std::memcpy(rhs + r0, c->rhs + r0, (size_t)(r1 - r0) * sizeof(double));
  return status(c, "rdc_csr_download_rows_async");
}
int rdc_ticket_wait(rdc_ctx* c, int ticket) {
  std::printf("wait %d\n", ticket);
  return status(c, "rdc_ticket_wait");
}
}
