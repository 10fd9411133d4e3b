"""CPU build (tests/host_solve_state_shim.cpp) of the two host-only pieces behind the linear-solve entries of the C-ABI.

The solver settings (rdcfes_amd/csrc/rdc_options.h, RDC_SOLVE_OPTIONS): the seven keys, their defaults, edge values, and every
refusal with its return code and message.

The validity rule (rdcfes_amd/csrc/rdc_solve_state.h): what csr_matvec_f32, mg_level, ilu_factor and gmres_stats may still hand
out after each kind of call, one group of cases per row of the table in DESIGN.md 2, each from a context where everything was
valid and from one where nothing was.

Every expectation is a literal (what the callers rely on); nothing is read back from the code under test."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RDC_OK, RDC_ERR_INVALID = 0, 1

# key -> (default, accepted values, refused values, message; {v} = the refused value)
SETTINGS = {
    "mg_omega": (600, [1, 2, 600, 1000, 1998, 1999], [0, -1, 2000, 100000, -2**31], "mg_omega is the damping in thousandths, 1 .. 1999, not {v}"),
    "mg_smoother": (0, [1, 0], [-1, 2, 7], "mg_smoother is 0 or 1, not {v}"),
    "mg_gs_fuse": (1, [0, 1], [-1, 2, 7], "mg_gs_fuse is 0 or 1, not {v}"),
    "ilu_factor_bits": (64, [32, 64], [0, 1, 16, 31, 33, 63, 65, 128, -32], "ilu_factor_bits is 64 or 32, not {v}"),
    "solve_method": (0, [1, 0], [-1, 2, 3], "solve_method is 0 (BiCGStab) or 1 (GMRES), not {v}"),
    "gmres_restart": (30, [1, 2, 30, 127, 128], [0, -1, 129, 1000, 2**31 - 1], "gmres_restart is 1 .. 128, not {v}"),
    "gmres_refine": (0, [1, 0], [-1, 2, 7], "gmres_refine is 0 or 1, not {v}"),
}
TUNING_KEYS = ["occupancy", "block", "kernel", "interior_nodes", "part", "ev_lds"]


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_state_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_state_shim.cpp"
    csrc = ROOT / "rdcfes_amd" / "csrc"
    deps = [src, csrc / "rdc_options.h", csrc / "rdc_solve_state.h", ROOT / "include" / "rdc_assembly.h"]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_solve_options_new.restype = C.c_void_p
    lib.shim_solve_options_delete.argtypes = [C.c_void_p]
    lib.shim_solve_options_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.shim_solve_options_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.shim_solve_option_key.restype = C.c_char_p
    lib.shim_solve_option_known.argtypes = [C.c_char_p]
    lib.shim_tuning_options_set.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.shim_valid_apply.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.shim_valid_apply.restype = None
    return lib


class Settings:
    def __init__(self, lib):
        self.lib, self.o = lib, lib.shim_solve_options_new()

    def close(self):
        self.lib.shim_solve_options_delete(self.o)

    def set(self, key, value):
        err = C.create_string_buffer(b"untouched", 512)
        rc = self.lib.shim_solve_options_set(self.o, key.encode(), value, err, 512)
        return rc, err.value.decode()

    def get(self, key):
        found = C.c_int(0)
        v = self.lib.shim_solve_options_get(self.o, key.encode(), C.byref(found))
        assert found.value == 1, f"no member for key {key!r}"
        return v

    def snapshot(self):
        return {k: self.get(k) for k in SETTINGS}


@pytest.fixture
def settings(lib):
    s = Settings(lib)
    yield s
    s.close()


def test_the_solver_table_holds_exactly_the_seven_keys(lib):
    keys = [lib.shim_solve_option_key(i).decode() for i in range(lib.shim_solve_option_count())]
    assert keys == ["mg_omega", "mg_smoother", "mg_gs_fuse", "ilu_factor_bits", "solve_method", "gmres_restart", "gmres_refine"]
    assert set(keys) == set(SETTINGS)


def test_the_defaults(settings):
    assert settings.snapshot() == {"mg_omega": 600, "mg_smoother": 0, "mg_gs_fuse": 1, "ilu_factor_bits": 64, "solve_method": 0,
                                   "gmres_restart": 30, "gmres_refine": 0}


@pytest.mark.parametrize("key", sorted(SETTINGS))
def test_accepted_values_are_stored_as_given(settings, key):
    default, accepted, _, _ = SETTINGS[key]
    assert settings.get(key) == default
    for v in accepted:
        before = settings.snapshot()
        rc, err = settings.set(key, v)
        assert rc == RDC_OK and err == "untouched", (key, v, err)
        assert settings.get(key) == v
        after = settings.snapshot()
        before.pop(key), after.pop(key)
        assert after == before                    # no other setting moved


@pytest.mark.parametrize("key", sorted(SETTINGS))
def test_refusals_say_why_and_leave_every_stored_value(settings, key):
    default, accepted, refused, message = SETTINGS[key]
    for start in [default, accepted[0]]:
        assert settings.set(key, start)[0] == RDC_OK
        for v in refused:
            before = settings.snapshot()
            rc, err = settings.set(key, v)
            assert rc == RDC_ERR_INVALID, (key, v)
            assert err == message.format(v=v)
            assert settings.snapshot() == before and settings.get(key) == start


def test_a_key_of_one_table_never_lands_in_the_other(lib, settings):
    for key in TUNING_KEYS + ["const_rows", "", "mg_omega ", "Mg_omega", "gmres"]:
        before = settings.snapshot()
        assert lib.shim_solve_option_known(key.encode()) == 0
        rc, err = settings.set(key, 1)
        assert rc == RDC_ERR_INVALID and err == f"unknown option '{key}'"
        assert settings.snapshot() == before
    for key in SETTINGS:
        assert lib.shim_solve_option_known(key.encode()) == 1
        err = C.create_string_buffer(b"untouched", 512)
        assert lib.shim_tuning_options_set(key.encode(), 1, err, 512) == RDC_ERR_INVALID
        assert err.value.decode() == f"unknown option '{key}'"


def test_a_short_message_buffer_is_not_overrun(lib, settings):
    err = C.create_string_buffer(b"\x7f" * 32, 32)
    assert lib.shim_solve_options_set(settings.o, b"gmres_restart", 129, err, 8) == RDC_ERR_INVALID
    assert err.raw[:8] == b"gmres_r\x00" and err.raw[8:] == b"\x7f" * 24


# ---- the validity rule ----
SCALE_F32, SOLVE, ARNOLDI, MG_APPLY, ILU_APPLY, DIST, DIST_PLAN = range(7)
NONE, JACOBI, BLOCK_JACOBI, MULTIGRID, ILU0, ILU0_LOCAL = range(6)
CONVERGED, MAX_ITS, BAD_DIAGONAL = 0, 1, 3
# outcomes: (stage, ran, comm_failed, bad_blocks, reason); matrix_bits follows from the call (32 for a mixed one) unless OVERFLOW
REFUSED = (0, 0, 0, 0, CONVERGED)      # refused after entry
VIEW_FAILED = (1, 0, 0, 0, CONVERGED)  # an allocation or upload of the views failed
OK = (2, 1, 0, 0, CONVERGED)
NOT_CONVERGED = (2, 1, 0, 0, MAX_ITS)
BAD_BLOCKS = (2, 1, 0, 2, CONVERGED)   # the hooks and rdc_csr_scale_f32 count them
BAD_DIAG = (2, 1, 0, 0, BAD_DIAGONAL)  # the solves report them as a reason
OVERFLOW = "overflow"                  # a mixed call whose copy did not fit fp32: matrix_bits 64
HIP_ERROR = (2, 0, 0, 0, CONVERGED)
COMM_FAILED = (2, 1, 1, 0, CONVERGED)

# (row, entry, precond, mixed, gmres, outcome, valid afterwards from all-valid, ... from all-invalid); letters: f = the fp32 copy,
# m = the multigrid values, i = the ILU(0) factor, g = the figures of a GMRES solve
CASES = [
    ("scale_f32", SCALE_F32, BLOCK_JACOBI, 1, 0, OK, "fig", "f"),
    ("scale_f32", SCALE_F32, BLOCK_JACOBI, 1, 0, BAD_BLOCKS, "ig", ""),
    ("scale_f32", SCALE_F32, JACOBI, 1, 0, OVERFLOW, "ig", ""),
    ("scale_f32", SCALE_F32, NONE, 1, 0, HIP_ERROR, "ig", ""),
    ("scale_f32", SCALE_F32, NONE, 1, 0, VIEW_FAILED, "ig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 0, 0, OK, "fig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 0, 0, NOT_CONVERGED, "fig", ""),
    ("solve", SOLVE, MULTIGRID, 0, 0, REFUSED, "fig", ""),
    ("solve", SOLVE, MULTIGRID, 0, 0, OK, "fmig", "m"),
    ("solve", SOLVE, MULTIGRID, 0, 0, BAD_DIAG, "fmig", "m"),
    ("solve", SOLVE, MULTIGRID, 0, 0, HIP_ERROR, "fig", ""),
    ("solve", SOLVE, ILU0, 0, 0, OK, "fig", "i"),
    ("solve", SOLVE, ILU0_LOCAL, 0, 0, OK, "fig", "i"),
    ("solve", SOLVE, ILU0, 0, 0, BAD_DIAG, "fig", "i"),
    ("solve", SOLVE, ILU0, 0, 0, REFUSED, "fig", ""),
    ("solve", SOLVE, ILU0, 0, 0, VIEW_FAILED, "fg", ""),
    ("solve", SOLVE, ILU0, 0, 0, HIP_ERROR, "fg", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, OK, "fig", "f"),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, NOT_CONVERGED, "fig", "f"),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, BAD_DIAG, "ig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, OVERFLOW, "ig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, HIP_ERROR, "ig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 1, 0, REFUSED, "fig", ""),
    ("solve", SOLVE, MULTIGRID, 1, 0, OK, "fmig", "fm"),
    ("solve", SOLVE, MULTIGRID, 1, 0, VIEW_FAILED, "ig", ""),
    ("solve", SOLVE, ILU0, 1, 0, OK, "fig", "fi"),
    ("solve", SOLVE, BLOCK_JACOBI, 0, 1, OK, "fiG", "G"),
    ("solve", SOLVE, MULTIGRID, 1, 1, OK, "fmiG", "fmG"),
    ("solve", SOLVE, BLOCK_JACOBI, 0, 1, HIP_ERROR, "fig", ""),
    ("solve", SOLVE, BLOCK_JACOBI, 0, 1, REFUSED, "fig", ""),
    ("arnoldi", ARNOLDI, BLOCK_JACOBI, 0, 1, OK, "fig", ""),
    ("arnoldi", ARNOLDI, MULTIGRID, 0, 1, OK, "fmig", "m"),
    ("arnoldi", ARNOLDI, MULTIGRID, 0, 1, BAD_BLOCKS, "fmig", "m"),
    ("arnoldi", ARNOLDI, ILU0, 0, 1, OK, "fig", "i"),
    ("arnoldi", ARNOLDI, ILU0_LOCAL, 0, 1, BAD_BLOCKS, "fig", "i"),
    ("arnoldi", ARNOLDI, BLOCK_JACOBI, 1, 1, OK, "fig", "f"),
    ("arnoldi", ARNOLDI, MULTIGRID, 1, 1, BAD_BLOCKS, "mig", "m"),
    ("arnoldi", ARNOLDI, ILU0, 1, 1, OVERFLOW, "ig", "i"),
    ("arnoldi", ARNOLDI, ILU0, 1, 1, HIP_ERROR, "g", ""),
    ("arnoldi", ARNOLDI, MULTIGRID, 1, 1, REFUSED, "fig", ""),
    ("mg_apply", MG_APPLY, MULTIGRID, 0, 0, OK, "fmig", "m"),
    ("mg_apply", MG_APPLY, MULTIGRID, 0, 0, BAD_BLOCKS, "fmig", "m"),
    ("mg_apply", MG_APPLY, MULTIGRID, 1, 0, OK, "fmig", "fm"),
    ("mg_apply", MG_APPLY, MULTIGRID, 1, 0, BAD_BLOCKS, "mig", "m"),
    ("mg_apply", MG_APPLY, MULTIGRID, 1, 0, OVERFLOW, "mig", "m"),
    ("mg_apply", MG_APPLY, MULTIGRID, 1, 0, HIP_ERROR, "ig", ""),
    ("mg_apply", MG_APPLY, MULTIGRID, 1, 0, REFUSED, "fig", ""),
    ("ilu_apply", ILU_APPLY, NONE, 0, 0, OK, "fig", "i"),
    ("ilu_apply", ILU_APPLY, NONE, 0, 0, BAD_BLOCKS, "fig", "i"),
    ("ilu_apply", ILU_APPLY, NONE, 0, 0, HIP_ERROR, "fg", ""),
    ("ilu_apply", ILU_APPLY, NONE, 0, 0, VIEW_FAILED, "fg", ""),
    ("ilu_apply", ILU_APPLY, NONE, 0, 0, REFUSED, "fig", ""),
    ("dist", DIST, BLOCK_JACOBI, 0, 0, OK, "fig", ""),
    ("dist", DIST, MULTIGRID, 0, 0, OK, "fig", ""),
    ("dist", DIST, MULTIGRID, 1, 0, OK, "fig", "f"),
    ("dist", DIST, ILU0_LOCAL, 0, 0, OK, "fig", "i"),
    ("dist", DIST, ILU0_LOCAL, 0, 0, COMM_FAILED, "fg", ""),
    ("dist", DIST, ILU0_LOCAL, 0, 0, HIP_ERROR, "fg", ""),
    ("dist", DIST, ILU0_LOCAL, 1, 0, OK, "fig", "fi"),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, OK, "fig", "f"),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, BAD_DIAG, "ig", ""),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, OVERFLOW, "ig", ""),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, COMM_FAILED, "ig", ""),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, HIP_ERROR, "ig", ""),
    ("dist", DIST, BLOCK_JACOBI, 1, 0, REFUSED, "fig", ""),
    ("dist_plan", DIST_PLAN, NONE, 0, 0, REFUSED, "fig", ""),
]


def _apply(lib, start, entry, precond, mixed, gmres, outcome):
    overflow = outcome == OVERFLOW
    stage, ran, comm, bad, reason = OK if overflow else outcome
    bits = 32 if mixed and not overflow else 64
    flags = (C.c_int * 6)(*start)
    out = (C.c_int * 7)(ran, comm, bad, bits, reason, 45, 6)   # the figures of this call, if it is a GMRES solve
    lib.shim_valid_apply(flags, entry, precond, mixed, gmres, stage, out)
    return tuple(flags)


def _flags(letters, old):
    """letters -> the six flags; g = the figures a GMRES solve left before (old), G = those of this call"""
    figures = (45, 6) if "G" in letters else old
    return (int("f" in letters), int("m" in letters), int("i" in letters), int("g" in letters.lower())) + figures


@pytest.mark.parametrize("row", sorted({c[0] for c in CASES}))
def test_validity_rule(lib, row):
    cases = [c for c in CASES if c[0] == row]
    assert cases
    for _, entry, precond, mixed, gmres, outcome, from_valid, from_invalid in cases:
        what = (row, precond, mixed, gmres, outcome)
        assert _apply(lib, (1, 1, 1, 1, 7, 3), entry, precond, mixed, gmres, outcome) == _flags(from_valid, (7, 3)), what
        assert _apply(lib, (0, 0, 0, 0, 0, 0), entry, precond, mixed, gmres, outcome) == _flags(from_invalid, (0, 0)), what
