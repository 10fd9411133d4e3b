"""A/B of the TET4 cluster kernel k_tet4_cl (rdc_tet4_cluster_mode) against the path the context takes without it, in one
process, on one context per mesh:

  * meshes.delaunay(n): the unstructured mesh (rows of up to ~50 node blocks: no pair lists, no element-visit lists), where
    mode 0 runs k_tet4_rowgather (PIHNA, RIPF, HCC) or k_rowgather<M, 4> (ADPM, PROTEAS) and mode 1 the cluster kernel;
  * Kuhn K(k), the regular-mesh control, where mode 0 runs the established kernels (k_tet4_ev, k_tet4_evc, k_tet4_rg5) and
    mode 2 forces the cluster kernel.

    python tools/tet4_cl_ab.py [--n 56] [--kuhn 60] [--rounds 10] [--reps 50] [--order -1|0|1] [--out profiles/tet4_cl_ab.txt]

Per case every shape is warmed up, then `rounds` rounds alternate three arms -- mode 0, the cluster kernel, mode 0 again -- of
`reps` assemblies each between two device events (whole assemble calls: the parent's record pack is part of its arm).  Reported
per arm: median and min .. max over the rounds of the time per assembly.  The difference of the medians of the two mode-0
arms is the run's noise floor: a difference between the cluster kernel and mode 0 (both arms pooled) below it is reported as
"no difference".  HBM fraction = algorithmic bytes (bench.algorithmic_bytes, the count of DESIGN.md section 4) over the median
time, of 8 TB/s.  Also printed: clusters, pairs per element visit, dynamic LDS, and registers / waves per SIMD of the
instantiation from lib/kernel_resources.json.  --order: "solid_cl_order" (pair order of the lists), -1 = the default."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

CASES = [("pihna", "shipped"), ("pihna", "full"), ("proteas", "full"), ("ripf", "shipped"), ("ripf", "full"), ("hcc", "full"),
         ("adpm", "full")]   # ordered by unknowns per node: one upload for five, one for three
NV = {"pihna": 5, "ripf": 3, "hcc": 3, "adpm": 3, "proteas": 5}
NAUX = {"pihna": 0, "ripf": 3, "hcc": 0, "adpm": 0, "proteas": 3}
# the instantiation launch_specialised picks (default options) and its fast exponent mode
KERNEL_CLASS = {("pihna", "shipped"): ("PihnaNoCellTransportMoments", 3), ("pihna", "full"): ("Pihna", 3),
                ("ripf", "shipped"): ("RipfReduced", 25), ("ripf", "full"): ("Ripf", 25), ("hcc", "full"): ("Hcc", 3),
                ("adpm", "full"): ("Adpm", 1), ("proteas", "full"): ("Proteas", 1)}


def _resources(model, pv):
    try:
        res = json.loads((ROOT / "rdcfes_amd" / "lib" / "kernel_resources.json").read_text())
    except OSError:
        return None
    cls, _ = KERNEL_CLASS[(model, pv)]
    hits = {k: v for k, v in res.items() if f"9k_tet4_clINS_{len(cls)}{cls}E" in k}
    return hits or None


def _inputs(model, pv, conn, xyz):
    import meshes
    from rdcfes_amd import (adpm_params_from_dict, hcc_params_from_dict, pihna_params_from_dict, proteas_params_from_dict,
                            ripf_params_from_dict, synth)
    from rdcfes_amd.context import FIELD_AUX_NODAL, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION
    f = meshes.unit_cube(xyz)
    if model == "pihna":
        return pihna_params_from_dict(synth.pihna_param_dict(pv)), {FIELD_OLD_SOLUTION: synth.pihna_fields(f)}
    if model == "ripf":
        u, aux = synth.ripf_fields(f)
        return ripf_params_from_dict(synth.ripf_param_dict(pv)), {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}
    if model == "hcc":
        return hcc_params_from_dict(synth.hcc_param_dict(pv)), {FIELD_OLD_SOLUTION: synth.hcc_fields(f)}
    if model == "adpm":
        u, tracts = synth.adpm_fields(f, conn.shape[0])
        return adpm_params_from_dict(synth.adpm_param_dict(pv), time=3.0), {FIELD_OLD_SOLUTION: u, FIELD_ELEM_TRACTS: tracts}
    u, aux = synth.proteas_fields(f)
    return proteas_params_from_dict(synth.proteas_param_dict(pv)), {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}


def _arm(torch, call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _fmt(x):
    return f"{np.median(x):8.4f} ({min(x):.4f} .. {max(x):.4f})"


def run_mesh(label, conn, xyz, on_mode, args, say):
    import torch
    from bench import HBM_PEAK_GBPS, algorithmic_bytes
    from rdcfes_amd import AssemblyContext
    say(f"\n== {label}: {conn.shape[0]} tets, {xyz.shape[0]} nodes; cluster kernel = mode {on_mode} ==")
    say(f"{'case':16s} {'mode 0 [ms]':>28s} {'cluster kernel [ms]':>28s} {'mode 0 again [ms]':>28s} {'noise':>7s} {'ratio':>6s}  "
        f"{'HBM frac 0 / cl':>15s}  verdict")
    rows = []
    with AssemblyContext(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        if args.order >= 0:
            ctx.set_option("solid_cl_order", args.order)
        nv_up = 0
        for model, pv in CASES:
            nv = NV[model]
            if nv != nv_up:
                t0 = time.time()
                ctx.mesh_upload(4, conn, xyz, nv)
                nv_up = nv
                say(f"-- upload with {nv} unknowns: {time.time() - t0:.1f} s host preparation")
            p, fields = _inputs(model, pv, conn, xyz)
            for f, a in fields.items():
                ctx.field_upload(f, a)
            call = {"pihna": ctx.assemble_pihna, "ripf": ctx.assemble_ripf, "hcc": ctx.assemble_hcc, "adpm": ctx.assemble_adpm,
                    "proteas": ctx.assemble_proteas}[model]
            vals = {}
            for mode in (0, on_mode):                    # warm up every shape (and build the lists), keep the results
                ctx.set_tet4_cluster(mode)
                for _ in range(3):
                    call(p)
                ctx.synchronize()
                info = ctx.tet4_cluster_info()
                if info["active"] != (1 if mode else 0):
                    raise RuntimeError(f"{model}/{pv}: mode {mode} gave active = {info['active']} ({info['last_error']})")
                vals[mode] = ctx.csr_download()
            err = max(np.linalg.norm(vals[on_mode][i] - vals[0][i]) / max(np.linalg.norm(vals[0][i]), 1e-300) for i in (0, 1))
            t = {"a": [], "b": [], "a2": []}
            for _ in range(args.rounds):
                for arm, mode in (("a", 0), ("b", on_mode), ("a2", 0)):
                    ctx.set_tet4_cluster(mode)
                    call(p)                              # the switch itself is not timed
                    t[arm].append(_arm(torch, lambda: call(p), args.reps))
            _, nnz = ctx.csr_dims()
            b_alg = algorithmic_bytes(4, conn.shape[0], xyz.shape[0], xyz.shape[0], nv, nv + NAUX[model], nnz)
            if model == "adpm":
                b_alg += 8 * 3 * conn.shape[0]           # the tract vectors
            m0, mb = float(np.median(t["a"] + t["a2"])), float(np.median(t["b"]))
            noise = abs(float(np.median(t["a"])) - float(np.median(t["a2"])))
            verdict = "no difference" if abs(mb - m0) <= noise else ("cluster kernel faster" if mb < m0 else "cluster kernel SLOWER")
            frac = lambda ms: b_alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
            say(f"{model + ' ' + pv:16s} {_fmt(t['a']):>28s} {_fmt(t['b']):>28s} {_fmt(t['a2']):>28s} {noise:7.4f} {m0 / mb:6.2f}  "
                f"{frac(m0):6.3f} / {frac(mb):6.3f}  {verdict}   (max rel. difference of the results {err:.1e})")
            rows.append((model, pv, info, _resources(model, pv)))
    say("lists and kernel resources:")
    for model, pv, info, res in rows:
        line = (f"  {model + ' ' + pv:16s} clusters {info['n_clusters']}, pairs {info['n_pairs']}, element visits {info['n_elem_visits']} "
                f"({info['n_pairs'] / max(info['n_elem_visits'], 1):.2f} pairs per visit), dynamic LDS {info['lds_bytes']} B")
        if res:
            line += "; " + ", ".join(f"{v.get('vgprs')} VGPRs, {v.get('scratch_bytes_per_lane', 0)} B scratch, {v.get('waves_per_simd')} waves/SIMD"
                                     for _, v in sorted(res.items()))
        say(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=56, help="meshes.delaunay(n)")
    ap.add_argument("--kuhn", type=int, default=60, help="Kuhn K(k), the regular-mesh control (0 = skip)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--order", type=int, default=-1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tet4_cl_ab.txt"))
    args = ap.parse_args()
    import meshes
    from rdcfes_amd import synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/tet4_cl_ab.py --n {args.n} --kuhn {args.kuhn} --rounds {args.rounds} --reps {args.reps} --order {args.order}")
    say("times: ms per assemble call, median (min .. max) over the rounds; ratio = mode 0 / cluster kernel")
    t0 = time.time()
    conn, xyz = meshes.delaunay(n=args.n)
    say(f"meshes.delaunay(n={args.n}) generated in {time.time() - t0:.1f} s")
    run_mesh(f"meshes.delaunay(n={args.n})", conn, xyz, 1, args, say)
    if args.kuhn > 0:
        conn, xyz = synth.kuhn_tet_mesh(args.kuhn, order="lex")
        run_mesh(f"Kuhn K({args.kuhn})", conn, xyz, 2, args, say)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
