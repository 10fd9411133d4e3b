"""CPU build of rdcfes_amd/csrc/rdc_options.h (tests/host_options_shim.cpp): the table behind rdc_set_option -- every key's
default, what is stored for an accepted value, and every refusal with its return code and message.  The expectations below
are literals (what the callers of rdc_set_option rely on); nothing is read back from the table under test."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RDC_OK, RDC_ERR_INVALID = 0, 1

# key -> (default, [(input, stored)])
ANY = [(0, 0), (1, 1), (-5, -5), (123456, 123456)]
FLAG = [(0, 0), (1, 1), (7, 1), (-1, 1)]
ACCEPTED = {
    "occupancy": (2, ANY), "ablate": (0, ANY), "specialise": (1, ANY), "lds_pad": (0, ANY), "stagger": (0, ANY),
    "moments": (1, ANY), "staged": (1, ANY), "xcd": (0, ANY), "schedule": (1, ANY), "grid": (0, ANY), "prefetch": (0, ANY),
    "solid_store": (0, ANY), "ev_occupancy": (3, ANY), "ev_lds": (54000, ANY),
    "interior_nodes": (-1, ANY + [(2**31 - 1, 2**31 - 1), (-2**31, -2**31)]),
    "solid_gather": (0, FLAG), "solid_split": (1, FLAG), "ev_background": (1, FLAG), "ev_general": (1, FLAG),
    "ev_resident": (1, [(2, 2), (5, 1), (0, 0), (-1, 1), (1, 1), (3, 1)]),
    "evc_occupancy": (2, [(3, 3), (7, 2), (2, 2), (0, 2), (-3, 2), (4, 2)]),
    "solid_cl_order": (-1, [(-3, -1), (0, 0), (9, 1), (-1, -1), (1, 1)]),
    "block": (256, [(128, 128), (256, 256)]),
    "part": (0, [(0, 0), (1, 1), (2, 2)]),
    "solid_kernel": (0, [(0, 0), (1, 1), (2, 2), (3, 3)]),
    "hex_kernel": (0, [(0, 0), (1, 1), (2, 2)]),
    "solid_cl_waves": (31, [(31, 31), (62, 62)]),
    "kernel": (0, [(0, 0), (1, 1), (2, 2), (3, 3), (5, 5), (7, 7)]),
}
# key -> (refused inputs, message; {v} = the refused value)
REFUSED = {
    "block": ([0, 64, 127, 129, 255, 257, 512, -128], "block must be 128 or 256"),
    "part": ([-1, 3, 100], "part must be 0, 1 or 2"),
    "solid_kernel": ([-1, 4, 100], "solid_kernel must be 0 (default), 1 (coloured), 2 (two-pass) or 3 (fused cluster kernel)"),
    "hex_kernel": ([-1, 3, 100], "hex_kernel must be 0 (cluster kernel), 1 (pair kernels) or 2 (persistent cluster kernel)"),
    "solid_cl_waves": ([0, 30, 32, 61, 63, 13, -31], "solid_cl_waves must be 31 (3 consumer + 1 producer waves) or 62"),
    "kernel": ([-1, 4, 6, 8, 99], "kernel must be 0, 1, 2, 3, 5 or 7, not {v}"),
}


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_options_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_options_shim.cpp"
    deps = [src, ROOT / "rdcfes_amd" / "csrc" / "rdc_options.h", ROOT / "include" / "rdc_assembly.h"]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_options_new.restype = C.c_void_p
    lib.shim_options_delete.argtypes = [C.c_void_p]
    lib.shim_options_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.shim_options_get.restype = C.c_int64
    lib.shim_options_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.shim_option_key.restype = C.c_char_p
    return lib


class Opts:
    def __init__(self, lib):
        self.lib, self.o = lib, lib.shim_options_new()

    def close(self):
        self.lib.shim_options_delete(self.o)

    def set(self, key, value):
        err = C.create_string_buffer(b"untouched", 512)
        rc = self.lib.shim_options_set(self.o, key.encode(), value, err, 512)
        return rc, err.value.decode()

    def get(self, key):
        nbytes = C.c_int(0)
        v = self.lib.shim_options_get(self.o, key.encode(), C.byref(nbytes))
        assert nbytes.value in (4, 8), f"no member for key {key!r}"
        return v

    def snapshot(self):
        return {k: self.get(k) for k in ACCEPTED}


@pytest.fixture
def opts(lib):
    o = Opts(lib)
    yield o
    o.close()


def test_the_table_holds_exactly_the_28_keys(lib):
    keys = [lib.shim_option_key(i).decode() for i in range(lib.shim_option_count())]
    assert len(keys) == 28 and len(set(keys)) == 28
    assert set(keys) == set(ACCEPTED)
    assert set(REFUSED) <= set(ACCEPTED)


@pytest.mark.parametrize("key", sorted(ACCEPTED))
def test_default_and_accepted_values(opts, key):
    default, cases = ACCEPTED[key]
    assert opts.get(key) == default
    assert len(cases) >= 2
    for value, stored in cases:
        before = opts.snapshot()
        rc, err = opts.set(key, value)
        assert rc == RDC_OK, (key, value, err)
        assert err == "untouched"                 # an accepted value writes no message
        assert opts.get(key) == stored, (key, value)
        after = opts.snapshot()
        before.pop(key), after.pop(key)
        assert after == before                    # ... and touches no other option


def test_interior_nodes_is_stored_in_64_bits(lib, opts):
    nbytes = C.c_int(0)
    lib.shim_options_get(opts.o, b"interior_nodes", C.byref(nbytes))
    assert nbytes.value == 8
    for key in ACCEPTED:
        if key != "interior_nodes":
            lib.shim_options_get(opts.o, key.encode(), C.byref(nbytes))
            assert nbytes.value == 4, key


@pytest.mark.parametrize("key", sorted(REFUSED))
def test_refusals_keep_the_stored_value(opts, key):
    values, message = REFUSED[key]
    for start in sorted({ACCEPTED[key][0], ACCEPTED[key][1][0][1], ACCEPTED[key][1][-1][1]}):   # from the default and from values set before
        assert opts.set(key, start)[0] == RDC_OK
        for v in values:
            before = opts.snapshot()
            rc, err = opts.set(key, v)
            assert rc == RDC_ERR_INVALID, (key, v)
            assert err == message.format(v=v)
            assert opts.snapshot() == before and opts.get(key) == start


@pytest.mark.parametrize("key", ["slim", "", "Kernel", "kernel ", "opt_kernel", "interior"])
def test_unknown_keys_are_refused_by_name(opts, key):
    before = opts.snapshot()
    rc, err = opts.set(key, 1)
    assert rc == RDC_ERR_INVALID
    assert err == f"unknown option '{key}'"
    assert opts.snapshot() == before


def test_a_short_message_buffer_is_not_overrun(lib, opts):
    err = C.create_string_buffer(b"\x7f" * 32, 32)
    assert lib.shim_options_set(opts.o, b"kernel", 99, err, 8) == RDC_ERR_INVALID
    assert err.raw[:8] == b"kernel \x00" and err.raw[8:] == b"\x7f" * 24
