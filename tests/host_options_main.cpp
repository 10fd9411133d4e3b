// Stand-alone driver of rdcfes_amd/csrc/rdc_options.h for a sanitizer build (tools/asan_options.sh): every key with values
// around each rule's edges, unknown and over-long keys, and message buffers down to one byte.  Prints "ok" and returns 0.
#include <climits>
#include <string>

#include "../rdcfes_amd/csrc/rdc_options.h"

static bool same(const rdc::Options& a, const rdc::Options& b) {
#define SAME(name, type, def, check, store) if (a.name != b.name) return false;
  RDC_OPTIONS(SAME)
#undef SAME
  return true;
}

int main() {
  const int values[] = {INT_MIN, -3, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 31, 62, 99, 128, 256, 54000, INT_MAX};
  int n = 0, refused = 0, accepted = 0;
  const char* const* keys = rdc::option_keys(&n);
  for (size_t errlen : {(size_t)512, (size_t)16, (size_t)1}) {
    std::string err(errlen, '\0');
    rdc::Options o;
    for (int k = 0; k < n; k++)
      for (int v : values) {
        const rdc::Options before = o;
        const int rc = rdc::options_set(o, keys[k], v, &err[0], errlen);
        if (rc == RDC_OK) { accepted++; continue; }
        refused++;
        if (rc != RDC_ERR_INVALID || !same(before, o) || std::strlen(err.c_str()) >= errlen) return 1;
      }
    const std::string longkey(4000, 'k');
    for (const char* key : {"", "slim", "kernel ", longkey.c_str()})
      if (rdc::options_set(o, key, 1, &err[0], errlen) != RDC_ERR_INVALID || std::strlen(err.c_str()) >= errlen) return 2;
  }
  std::printf("ok: %d keys, %d values accepted, %d refused\n", n, accepted, refused);
  return n == 28 ? 0 : 3;
}
