// Stand-alone driver of rdcfes_amd/csrc/rdc_const_rows.h for a sanitizer build (tests/test_host_const_rows.py): the record "the a
// rows in memory are those of key K over parts P" through every transition the launch code makes, the decision (4 or 5 rows)
// asserted after each.  Prints "ok" and returns 0; a failed expectation prints its line and returns 1.
#include <cmath>
#include <cstdio>

#include "../rdcfes_amd/csrc/rdc_const_rows.h"

using namespace rdc;

namespace {
int failures = 0, checks = 0;
#define EXPECT(cond) do { checks++; if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

struct K { double Tsec_c, Tsec_h, Tdec, Tupt; };   // the members of PihnaK that const_rows_key reads
const K shipped{0.5e-3, 0.25e-3, 0.125e-3, 0.0};

// what assemble_rd does around a launch: decide, "launch", record
int step(ConstRows& r, int mode, const K& k, int part, int64_t interior, bool capturing = false, bool ok = true) {
  const ConstRowsKey key = const_rows_key(k);
  const int n = r.rows(mode, key, part, interior, capturing);
  r.launched(n, key, part, capturing, ok);
  return n;
}
}  // namespace

int main() {
  {  // the plain sequence: first launch writes, later ones skip, whatever the state; mode 0 never skips and keeps the record
    ConstRows r;
    r.mesh_upload();
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 4);
    EXPECT(step(r, 1, shipped, 0, -1) == 4);
    EXPECT(step(r, 0, shipped, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 4);
    EXPECT(step(r, 2, shipped, 0, -1) == 4);
  }
  {  // the key: dt (all three), one rate, the uptake
    ConstRows r;
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    K k = shipped; k.Tsec_c *= 2; k.Tsec_h *= 2; k.Tdec *= 2;
    EXPECT(step(r, 1, k, 0, -1) == 5);
    EXPECT(step(r, 1, k, 0, -1) == 4);
    EXPECT(step(r, 1, shipped, 0, -1) == 5);   // back: the rows hold the other key
    EXPECT(step(r, 1, shipped, 0, -1) == 4);
    K d = shipped; d.Tdec = 0.3;
    EXPECT(step(r, 1, d, 0, -1) == 5);
    EXPECT(step(r, 1, d, 0, -1) == 4);
    K s = shipped; s.Tsec_h = 0.0;
    EXPECT(step(r, 1, s, 0, -1) == 5);
    K u = shipped; u.Tupt = 1e-5;              // state-dependent rows: never skipped, and what they leave is no one's constant rows
    EXPECT(step(r, 1, u, 0, -1) == 5);
    EXPECT(step(r, 1, u, 0, -1) == 5);
    EXPECT(step(r, 2, u, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 4);
    K nan = shipped; nan.Tdec = std::nan("");   // a NaN equals nothing, itself included
    EXPECT(step(r, 1, nan, 0, -1) == 5);
    EXPECT(step(r, 1, nan, 0, -1) == 5);
  }
  {  // mesh and coordinates
    ConstRows r;
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    r.coords_update();
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    r.mesh_upload();
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    r.other_assembly();                         // another kernel path or model
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    EXPECT(step(r, 1, shipped, 0, -1, false, false) == 4);   // a failed launch: nothing is known any more
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    EXPECT(step(r, 1, shipped, 0, -1, true, false) == 5);    // ... a failed captured one too
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
  }
  {  // two parts: each part answers for its own rows, a whole assembly for both
    ConstRows r;
    const int64_t in = 100;
    EXPECT(step(r, 1, shipped, 1, in) == 5);
    EXPECT(step(r, 1, shipped, 1, in) == 4);
    EXPECT(step(r, 1, shipped, 0, in) == 5);    // part 2's rows were never written
    EXPECT(step(r, 1, shipped, 2, in) == 4);    // the whole assembly wrote them
    EXPECT(step(r, 1, shipped, 1, in) == 4);
    r.mesh_upload();
    EXPECT(step(r, 1, shipped, 2, in) == 5);
    EXPECT(step(r, 1, shipped, 1, in) == 5);
    EXPECT(step(r, 1, shipped, 1, in) == 4 && step(r, 1, shipped, 2, in) == 4 && step(r, 1, shipped, 0, in) == 4);
    // part 1 alone with another dt, then a whole assembly with it: part 2's rows still hold the old key
    K k = shipped; k.Tsec_c *= 3; k.Tsec_h *= 3; k.Tdec *= 3;
    EXPECT(step(r, 1, k, 1, in) == 5);
    EXPECT(step(r, 1, k, 1, in) == 4);
    EXPECT(step(r, 1, k, 0, in) == 5);
    EXPECT(step(r, 1, k, 2, in) == 4);
    // another split: the flags refer to other rows
    EXPECT(step(r, 1, k, 1, in + 1) == 5);
    EXPECT(step(r, 1, k, 2, in + 1) == 5);
    EXPECT(step(r, 1, k, 1, in + 1) == 4 && step(r, 1, k, 2, in + 1) == 4);
    EXPECT(step(r, 1, k, 0, -1) == 5);          // "interior_nodes" changed, a whole assembly or not
    EXPECT(step(r, 1, k, 0, -1) == 4);
    EXPECT(step(r, 1, k, 2, in) == 5);
  }
  {  // pointers in the caller's hands
    ConstRows r;
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    r.values_pointer();
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 2, shipped, 0, -1) == 4);    // the promise of mode 2 (the launches above kept the record)
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    r.mesh_upload();                            // a new value array: that pointer is void
    EXPECT(step(r, 1, shipped, 0, -1) == 5 && step(r, 1, shipped, 0, -1) == 4);
    r.coords_pointer();
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    r.mesh_upload();                            // ... the coordinates' is not: for the life of the context
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 1, shipped, 0, -1) == 5);
    EXPECT(step(r, 2, shipped, 0, -1) == 4);
    EXPECT(step(r, 0, shipped, 0, -1) == 5);
  }
  {  // captured launches write everything and leave the record; afterwards only their key may be skipped
    ConstRows r;
    const int64_t in = 50;
    EXPECT(step(r, 1, shipped, 1, in, true) == 5);
    EXPECT(step(r, 1, shipped, 2, in, true) == 5);
    EXPECT(!r.valid[0] && !r.valid[1]);         // a capture executes nothing
    EXPECT(step(r, 1, shipped, 1, in) == 5 && step(r, 1, shipped, 2, in) == 5);
    EXPECT(step(r, 1, shipped, 1, in) == 4 && step(r, 1, shipped, 2, in) == 4);
    EXPECT(step(r, 2, shipped, 1, in, true) == 5);
    EXPECT(r.valid[0] && r.valid[1]);
    K k = shipped; k.Tsec_c *= 2; k.Tsec_h *= 2; k.Tdec *= 2;
    EXPECT(step(r, 1, k, 0, in) == 5);
    EXPECT(step(r, 1, k, 0, in) == 5);          // a replay may have put the captured key's rows back at any time
    EXPECT(step(r, 2, k, 0, in) == 5);
    EXPECT(step(r, 1, shipped, 0, in) == 5);
    EXPECT(step(r, 1, shipped, 0, in) == 4);
    EXPECT(step(r, 1, k, 0, in, true) == 5);    // a second graph with another key: nothing can be skipped
    EXPECT(step(r, 1, shipped, 0, in) == 5 && step(r, 1, shipped, 0, in) == 5 && step(r, 1, k, 0, in) == 5 && step(r, 1, k, 0, in) == 5);
    r.mesh_upload();                            // the graphs died with the buffers they name
    EXPECT(step(r, 1, k, 0, in) == 5 && step(r, 1, k, 0, in) == 4);
  }
  {  // the option itself: 0, 1, 2 and nothing else; the default is 1 and no event of the record touches it
    EXPECT(!const_rows_mode_ok(-1) && const_rows_mode_ok(0) && const_rows_mode_ok(1) && const_rows_mode_ok(2) && !const_rows_mode_ok(3) && !const_rows_mode_ok(100));
    ConstRows r;
    EXPECT(r.mode == 1);
    r.mode = 2;
    r.mesh_upload(); r.coords_update(); r.other_assembly(); r.values_pointer(); r.coords_pointer();
    EXPECT(step(r, r.mode, shipped, 0, -1, false, false) == 5);
    EXPECT(r.mode == 2);
    EXPECT(step(r, r.mode, shipped, 0, -1) == 5 && step(r, r.mode, shipped, 0, -1) == 4);
  }
  if (failures) { std::printf("%d of %d expectations failed\n", failures, checks); return 1; }
  std::printf("ok: %d decisions\n", checks);
  return 0;
}
