"""Per-block parity of an assembled CSR system against the oracle's.

One relative norm over all CSR values is dominated by the largest (equation, unknown) block: in PIHNA the (v, a) block holds
essentially all of the Frobenius norm, so the n, c, h equations could be zeroed and a global 1e-10 would still pass.  Here
every block (a, b) -- the entries of rows node * nv + a and columns node * nv + b, the oracle's dof layout -- and every
rhs variable is compared on its own scale:

  ||B - B0|| / ||B0|| <= rtol                         where the oracle's block is not zero, however small
  ||B|| <= 1e-14 * max_b ||B0(a, b)||                 where it is exactly zero (a structural zero of equation a)
  ||r_a - r0_a|| / ||r0_a|| <= rtol                   rhs variable a; if the oracle's is exactly zero:
  ||r_a|| <= 1e-14 * max_b ||r0_b||

Entries that are NaN in the oracle (0/0 states) must be NaN in the result too and are left out of the norms.  Per-block
bounds of 1e-10 imply the global one, which the tests keep next to these checks.

A test may name blocks that the oracle itself does not reproduce (`noise_blocks`): values that are exact zeros plus
rounding, which change by O(1) with the order of the oracle's own sums.  Such a block is held to
||B - B0|| <= 1e-14 * max_b ||B0(a, b)||, and the test must show the oracle's own spread and give the measured values."""
import numpy as np

ZERO_REL = 1e-14     # a structurally zero (or named noise) block: at most this fraction of the largest block norm of its equation
MAX_RTOL = 1e-8      # no block may be given a looser relative bound than this
CHUNK = 1 << 24      # entries per slice of the chunked form


def _sq_blocks(rp, col, val, val0, nv, r_begin, r_end, acc_d, acc_0):
    """add the squared differences and oracle values of rows [r_begin, r_end) into the (a, b) accumulators"""
    e0, e1 = int(rp[r_begin]), int(rp[r_end])
    if e1 == e0:
        return
    rows = np.arange(r_begin, r_end, dtype=np.int64)
    eq = np.repeat(rows % nv, np.diff(rp[r_begin:r_end + 1]))
    key = eq * nv + np.asarray(col[e0:e1], dtype=np.int64) % nv
    v, v0 = val[e0:e1], val0[e0:e1]
    n0 = np.isnan(v0)
    if not np.array_equal(np.isnan(v), n0):
        bad = np.flatnonzero(np.isnan(v) != n0)[0]
        raise AssertionError(f"NaN pattern differs from the oracle's at CSR entry {e0 + bad} "
                             f"(equation {eq[bad]}, unknown {key[bad] % nv}): {v[bad]!r} vs {v0[bad]!r}")
    if n0.any():
        ok = ~n0
        key, v, v0 = key[ok], v[ok], v0[ok]
    d = v - v0
    acc_d += np.bincount(key, weights=d * d, minlength=nv * nv)
    acc_0 += np.bincount(key, weights=v0 * v0, minlength=nv * nv)


def block_norms(rp, col, val, val0, nv, chunk=None):
    """(||B - B0||, ||B0||) per block, each [nv, nv] indexed [equation, unknown]"""
    rp = np.asarray(rp)
    n_rows = rp.size - 1
    acc_d, acc_0 = np.zeros(nv * nv), np.zeros(nv * nv)
    if chunk is None:
        _sq_blocks(rp, col, val, val0, nv, 0, n_rows, acc_d, acc_0)
    else:
        r = 0
        while r < n_rows:
            r_end = int(np.searchsorted(rp, rp[r] + chunk, side="right")) - 1
            r_end = min(max(r_end, r + 1), n_rows)
            _sq_blocks(rp, col, val, val0, nv, r, r_end, acc_d, acc_0)
            r = r_end
    return np.sqrt(acc_d).reshape(nv, nv), np.sqrt(acc_0).reshape(nv, nv)


def _check(norm_d, norm_0, tol, noise, zero_scale, names, what):
    """norm_* [n_eq, n_unk]; tol [n_eq, n_unk]; noise: set of (a, b); zero_scale [n_eq]: the worst block first in the message"""
    worst, msgs = None, []
    for a in range(norm_0.shape[0]):
        for b in range(norm_0.shape[1]):
            if (a, b) in noise or norm_0[a, b] == 0.0:
                err = norm_d[a, b] / zero_scale[a] if zero_scale[a] > 0.0 else (np.inf if norm_d[a, b] > 0.0 else 0.0)
                bound, kind = ZERO_REL, "noise-block" if (a, b) in noise else "zero-block"
            else:
                err, bound, kind = norm_d[a, b] / norm_0[a, b], tol[a, b], "rel"
            if not err <= bound:        # NaN fails
                score = err / bound if np.isfinite(err) else np.inf
                msgs.append((score, f"{what}{names(a, b)}: {kind} error {err:.3e} > {bound:.1e}"))
                if worst is None or score > worst[0]:
                    worst = (score, msgs[-1][1])
    if msgs:
        msgs.sort(key=lambda m: -m[0])
        raise AssertionError(f"worst {worst[1]}" + ("" if len(msgs) == 1 else
                             f"; {len(msgs) - 1} more: " + "; ".join(m[1] for m in msgs[1:6])))


def _check_rhs(rhs, rhs0, nv, rtol, rhs_rtol):
    rhs, rhs0 = np.asarray(rhs).reshape(-1, nv), np.asarray(rhs0).reshape(-1, nv)
    n0 = np.isnan(rhs0)
    if not np.array_equal(np.isnan(rhs), n0):
        raise AssertionError("rhs NaN pattern differs from the oracle's")
    r, r0 = np.where(n0, 0.0, rhs), np.where(n0, 0.0, rhs0)
    norm_d = np.linalg.norm(r - r0, axis=0)[None, :]
    norm_0 = np.linalg.norm(r0, axis=0)[None, :]
    t = np.full((1, nv), float(rtol))
    for a, v in (rhs_rtol or {}).items():
        t[0, a] = v
    assert t.max() <= MAX_RTOL, f"a per-variable bound looser than {MAX_RTOL:g} is a bug to investigate, not a tolerance"
    # only an exactly zero rhs variable is measured against the largest rhs variable
    _check(norm_d, norm_0, t, set(), norm_0.max(axis=1), lambda a, b: f"rhs variable {b}", "")


def assert_csr_close(rp, col, val, val0, rhs, rhs0, nv, rtol=1e-10, block_rtol=None, rhs_rtol=None, noise_blocks=(),
                     chunk=None):
    """Every (equation, unknown) block of val and every rhs variable within rtol of the oracle's on its own norm.
    block_rtol {(a, b): bound} and rhs_rtol {a: bound} loosen single blocks (at most MAX_RTOL; say why where used);
    noise_blocks: blocks the oracle does not reproduce itself (see the module docstring).
    rp, col: the scalar CSR pattern of val0 (val on the same pattern); rhs / rhs0 may be None."""
    assert np.asarray(val).shape == np.asarray(val0).shape
    assert int(np.asarray(rp)[-1]) == np.asarray(val0).size
    t = np.full((nv, nv), float(rtol))
    for (a, b), r in (block_rtol or {}).items():
        t[a, b] = r
    assert t.max() <= MAX_RTOL, f"a per-block bound looser than {MAX_RTOL:g} is a bug to investigate, not a tolerance"
    norm_d, norm_0 = block_norms(rp, col, val, val0, nv, chunk=chunk)
    _check(norm_d, norm_0, t, set(noise_blocks), norm_0.max(axis=1), lambda a, b: f"block ({a}, {b})", "matrix ")
    if rhs is not None:
        _check_rhs(rhs, rhs0, nv, rtol, rhs_rtol)


def assert_csr_close_chunked(rp, col, val, val0, rhs, rhs0, nv, chunk=CHUNK, **kw):
    """assert_csr_close over slices of about `chunk` entries: no temporaries of the size of val (the K(119) system)"""
    assert_csr_close(rp, col, val, val0, rhs, rhs0, nv, chunk=chunk, **kw)
