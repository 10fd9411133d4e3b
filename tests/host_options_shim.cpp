// g++ build of rdcfes_amd/csrc/rdc_options.h for tests/test_host_options.py: the option table of rdc_set_option, callable
// from ctypes without a device.
#include "../rdcfes_amd/csrc/rdc_options.h"

extern "C" {

void* shim_options_new() { return new rdc::Options(); }
void shim_options_delete(void* o) { delete static_cast<rdc::Options*>(o); }

int shim_options_set(void* o, const char* key, int value, char* err, int errlen) {
  return rdc::options_set(*static_cast<rdc::Options*>(o), key, value, err, (size_t)errlen);
}

// stored value of a key; *bytes = width of its storage (0: no such member)
int64_t shim_options_get(const void* o, const char* key, int* bytes) {
  const rdc::Options& opt = *static_cast<const rdc::Options*>(o);
#define SHIM_GET(name, type, def, check, store) \
  if (!std::strcmp(key, #name)) { *bytes = (int)sizeof(opt.name); return (int64_t)opt.name; }
  RDC_OPTIONS(SHIM_GET)
#undef SHIM_GET
  *bytes = 0;
  return 0;
}

int shim_option_count() { int n = 0; rdc::option_keys(&n); return n; }
const char* shim_option_key(int i) { int n = 0; return rdc::option_keys(&n)[i]; }

}
