#!/usr/bin/env python3
"""Which kernels run: a matrix of small reaction-diffusion assemblies for a kernel trace ("Which kernel runs").

    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/path_matrix.py run LABELS.txt
    python tools/path_matrix.py reduce DIR/**/trace_kernel_trace.csv LABELS.txt OUT.txt

`run` assembles every case on a fresh context, with a launch of k_clamp_nonnegative on a scratch field in front of the call and
one behind it, so that the trace splits into cases and the uploads stay outside them; it writes one label per case with what
the call reported (error code, rdc_part1_nodes before / after, rdc_tet4_cluster_info).  `reduce` joins the two: every distinct
sequence of kernel names (launch order, "xN" = N launches in a row) with the cases that ran it, and one digest over the full
detail (per case the grid, workgroup size and LDS bytes of every launch, and what the call reported).  Two commits run the same
kernels with the same launch sizes when their files are equal.  Only API that predates the path header (rdc_path.h) is used,
so the script runs unchanged on older commits."""
import csv
import hashlib
import re
import sys
import textwrap
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SEPARATOR = "k_clamp_nonnegative"
MODELS = [("pihna", "shipped"), ("pihna", "full"), ("pihna", "realexp"), ("ripf", "shipped"), ("ripf", "full"), ("hcc", "shipped"),
          ("hcc", "full"), ("adpm", "shipped"), ("adpm", "full"), ("proteas", "full")]
NV = {"pihna": 5, "ripf": 3, "hcc": 3, "adpm": 3, "proteas": 5}
# tests/test_gpu_parity.py, _PIHNA_OPTION_SETS
PIHNA_OPTION_SETS = [{"kernel": 7}, {"kernel": 7, "ev_occupancy": 2}, {"kernel": 5}, {"kernel": 5, "occupancy": 3}, {"kernel": 3}, {"kernel": 2},
                     {"kernel": 1}, {"occupancy": 1}, {"xcd": 1}, {"prefetch": 16}, {"specialise": 0}, {"moments": 0}, {"stagger": 8},
                     {"ev_resident": 0}, {"ev_resident": 0, "kernel": 7}, {"ev_resident": 2}, {"ev_resident": 1, "grid": 7},
                     {"ev_resident": 1, "grid": 1}, {"ev_resident": 1, "grid": 100000}]
# the other knobs that move a call from one kernel family to another
KNOBS = [{"ablate": 1}, {"ablate": 4}, {"kernel": 7, "ablate": 4}, {"kernel": 5, "ablate": 2}, {"lds_pad": 8}, {"ev_general": 0},
         {"ev_general": 0, "specialise": 0}, {"specialise": 0, "moments": 0}, {"block": 128}, {"block": 128, "kernel": 3}, {"occupancy": 3},
         {"kernel": 1, "occupancy": 1, "ablate": 1}, {"kernel": 2, "occupancy": 3}, {"kernel": 3, "occupancy": 1}, {"staged": 0}, {"staged": 2}]


def _meshes():
    import meshes
    from rdcfes_amd import partition, synth
    out = {}
    for n, order in ((7, "random"), (8, "random"), (9, "lex"), (10, "random"), (11, "lex"), (12, "lex")):
        conn, xyz = synth.kuhn_tet_mesh(n, order=order)
        out[f"K{n}"] = (4, conn, xyz, xyz, xyz.shape[0], int(0.6 * xyz.shape[0]))
    conn, xyz = synth.hex_mesh(5, jitter=0.15, order="random")
    out["H5"] = (8, conn, xyz, xyz, xyz.shape[0], int(0.6 * xyz.shape[0]))
    conn, xyz = synth.kuhn_tet_mesh(8, order="random")          # the ghosted partition of tests/test_host_parts.py
    lp = partition.build_local(conn, xyz, partition.partition_rcb(xyz[conn].mean(axis=1), 3), 1, 3)
    out["ghost"] = (4, lp.conn, lp.xyz, lp.xyz, lp.n_owned, lp.n_interior)
    conn, xyz = meshes.hydrogel()
    out["hydrogel"] = (4, conn, xyz, meshes.unit_cube(xyz), xyz.shape[0], int(0.6 * xyz.shape[0]))
    return out


def _inputs(model, pv, fxyz, n_elem):
    """(parameter struct, {field: array})"""
    from rdcfes_amd import (adpm_params_from_dict, hcc_params_from_dict, pihna_params_from_dict, proteas_params_from_dict,
                            ripf_params_from_dict, synth)
    from rdcfes_amd.context import FIELD_AUX_NODAL, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION
    if model == "pihna":
        return pihna_params_from_dict(synth.pihna_param_dict(pv)), {FIELD_OLD_SOLUTION: synth.pihna_fields(fxyz)}
    if model == "ripf":
        u, aux = synth.ripf_fields(fxyz)
        return ripf_params_from_dict(synth.ripf_param_dict(pv)), {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}
    if model == "hcc":
        return hcc_params_from_dict(synth.hcc_param_dict(pv)), {FIELD_OLD_SOLUTION: synth.hcc_fields(fxyz)}
    if model == "adpm":
        u, tracts = synth.adpm_fields(fxyz, n_elem)
        return adpm_params_from_dict(synth.adpm_param_dict(pv), time=3.0), {FIELD_OLD_SOLUTION: u, FIELD_ELEM_TRACTS: tracts}
    u, aux = synth.proteas_fields(fxyz)
    return proteas_params_from_dict(synth.proteas_param_dict(pv)), {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}


# what moves a model other than PIHNA between families beside "kernel"
OTHER_KNOBS = [{"ablate": 1}, {"lds_pad": 8}, {"ev_general": 0}, {"block": 128}, {"block": 128, "kernel": 3}, {"staged": 0}, {"staged": 2}]


def cases():
    """(mesh, model, parameter variant, strategy, kernel variant, options, cluster mode, parts, stamps armed)"""
    out = []
    add = lambda *c: out.append(c)
    for mv in MODELS:
        for mesh in ("K9", "H5", "hydrogel"):                                   # strategy x variant, default options
            for strategy in (0, 1, 2):
                for variant in (0, 1):
                    add(mesh, *mv, strategy, variant, {}, 0, (0,), False)
        for mesh in ("K7", "K8", "K10", "K11", "K12", "ghost"):
            add(mesh, *mv, 0, 0, {}, 0, (0,), False)
        for mesh in ("K12", "ghost", "H5", "hydrogel"):                          # the two parts of the default path
            add(mesh, *mv, 0, 0, {}, 0, (1, 2), False)
        for kernel in (0, 1, 2, 3, 5, 7):                                        # "kernel", whole and in two parts
            add("K9", *mv, 0, 0, {"kernel": kernel}, 0, (0,), False)
            add("K12", *mv, 0, 0, {"kernel": kernel}, 0, (1, 2), False)
        for hk in (0, 1, 2):                                                     # "hex_kernel", "solid_cl_waves"
            add("H5", *mv, 0, 0, {"hex_kernel": hk}, 0, (0,), False)
            add("H5", *mv, 0, 0, {"hex_kernel": hk}, 0, (1, 2), False)
        add("H5", *mv, 0, 0, {"solid_cl_waves": 62}, 0, (0,), False)
        for mode in (1, 2):                                                      # rdc_tet4_cluster_mode (0: every other case)
            for mesh in ("K7", "ghost", "hydrogel"):
                add(mesh, *mv, 0, 0, {}, mode, (0,), False)
                add(mesh, *mv, 0, 0, {}, mode, (1, 2), False)
            add("hydrogel", *mv, 1, 0, {}, mode, (0,), False)
            add("hydrogel", *mv, 0, 1, {}, mode, (0,), False)
            add("K7", *mv, 0, 0, {"kernel": 3}, mode, (0,), False)
        for opts in (KNOBS if mv[0] == "pihna" else OTHER_KNOBS):
            add("K9", *mv, 0, 0, opts, 0, (0,), False)
    for pv in ("shipped", "full"):
        for opts in PIHNA_OPTION_SETS:
            add("K9", "pihna", pv, 0, 0, opts, 0, (0,), False)
            add("K12", "pihna", pv, 0, 0, opts, 0, (1, 2), False)
        for opts in KNOBS:
            add("K12", "pihna", pv, 0, 0, opts, 0, (1, 2), False)
        for opts in ({}, {"kernel": 3}, {"kernel": 7, "ablate": 4}):            # armed stamps (tools/stamp_report.py, tools/ev_timeline.py)
            add("K9", "pihna", pv, 0, 0, opts, 0, (0,), True)
    return out


def run(labels_path):
    import ctypes as C
    import numpy as np
    from rdcfes_amd import AssemblyContext, RdcError
    from rdcfes_amd.context import FIELD_PREV_SOLUTION
    meshes = _meshes()
    inputs = {}
    with open(labels_path, "w") as labels:
        for mesh, model, pv, strategy, variant, opts, mode, parts, stamps in cases():
            nen, conn, xyz, fxyz, n_owned, n_interior = meshes[mesh]
            if (mesh, model, pv) not in inputs:
                inputs[(mesh, model, pv)] = _inputs(model, pv, fxyz, conn.shape[0])
            p, fields = inputs[(mesh, model, pv)]
            with AssemblyContext(0) as ctx:
                assemble = getattr(ctx, "assemble_" + model)
                status = []
                try:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    if parts != (0,):
                        ctx.set_option("interior_nodes", n_interior)
                    if mode:
                        ctx.set_tet4_cluster(mode)
                    ctx.mesh_upload(nen, conn, xyz, NV[model], n_owned=n_owned)
                    ctx.set_scatter(strategy)
                    ctx.set_kernel_variant(variant)
                    for f, a in fields.items():
                        ctx.field_upload(f, a)
                    ctx.field_upload(FIELD_PREV_SOLUTION, np.zeros(xyz.shape[0] * NV[model]))
                    if stamps:
                        ctx._ck(ctx._lib.rdc_debug_stamps(ctx._h, None, 0, C.byref(C.c_int64())))
                    ctx.synchronize()
                except RdcError as e:
                    status.append(f"setup error {e.code}")
                    parts = ()
                for part in parts:
                    what = f"part={part}"
                    try:
                        if part:
                            what += f" predicted={ctx.part1_nodes()}"
                        ctx.set_option("part", part)
                        ctx.clamp_nonnegative(FIELD_PREV_SOLUTION)     # the separator in front: uploads stay outside the case
                        assemble(p)
                        what += f" ok part1_nodes={ctx.part1_nodes()}" if part else " ok"
                    except RdcError as e:
                        what += f" error {e.code}"
                    info = ctx.tet4_cluster_info()
                    what += f" cl_active={info['active']} cl_lds={info['lds_bytes']} cl_clusters={info['n_clusters']}"
                    ctx.set_option("part", 0)
                    ctx.clamp_nonnegative(FIELD_PREV_SOLUTION)     # the separator behind
                    ctx.synchronize()
                    status.append(what)
                o = ",".join(f"{k}={v}" for k, v in opts.items()) or "-"
                head = f"{mesh} {model}/{pv} strategy={strategy} variant={variant} cl_mode={mode} stamps={int(stamps)} opts={o}"
                for s in status:
                    labels.write(f"{head} | {s}\n")
                labels.flush()
    print("cases written:", labels_path)


def _short(name):
    """kernel name with its template arguments, without namespace, return type and parameter list"""
    m = re.match(r"(?:void )?([\w:]+)(<.*>)?\(", name + "(")
    return ((m.group(1) + (m.group(2) or "")) if m else name).replace("rdc::", "")


def _case(label):
    """the label of `run` in short: defaults left out"""
    head, status = label.split(" | ")
    f = head.split()
    kv = dict(t.split("=", 1) for t in f[2:])
    words = f[:2] + [w for w in (("", "coloured", "rowgather")[int(kv["strategy"])], "generic" * int(kv["variant"]),
                                 f"cluster_mode={kv['cl_mode']}" * (kv["cl_mode"] != "0"), "stamps" * int(kv["stamps"]),
                                 kv["opts"] if kv["opts"] != "-" else "") if w]
    m = re.search(r"part=(\d)(?: predicted=\d+)? (ok|error \d+)(?: part1_nodes=(\d+))?", status)
    if m.group(1) != "0":
        words.append(f"part={m.group(1)}" + (f"->{m.group(3)}" if m.group(1) == "1" and m.group(3) else ""))
    if m.group(2) != "ok":
        words.append(m.group(2))
    return " ".join(words[:2]), " ".join(words[2:]) or "default"


def reduce(trace_csv, labels_path, out_path):
    rows = list(csv.DictReader(open(trace_csv, newline="")))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], []
    for r in rows:
        name = _short(r["Kernel_Name"])
        if name.startswith("__amd_rocclr_copyBuffer"):            # the runtime's copies of the uploads
            continue
        if name == SEPARATOR:
            groups.append(cur)
            cur = []
        else:
            cur.append((name, f"{r['Grid_Size_X']}/{r['Workgroup_Size_X']}/{r['LDS_Block_Size']}"))
    labels = [ln.rstrip("\n") for ln in open(labels_path)]
    # rdc_part1_nodes before the first part-1 call is a prediction, which a commit may improve: it is reported, not compared
    wrong = [ln for ln in labels if (m := re.search(r"part=1 predicted=(\d+) ok part1_nodes=(\d+)", ln)) and m.group(1) != m.group(2)]
    print(f"{len(wrong)} part-1 calls completed other rows than rdc_part1_nodes predicted before them")
    for ln in wrong:
        print("  " + ln)
    labels = [re.sub(r" predicted=\d+", "", ln) for ln in labels if "setup error" not in ln]
    calls = groups[1::2]                                          # [uploads] separator [the call] separator ...
    ok = len(groups) == 2 * len(labels) and not cur
    by_seq, detail = {}, hashlib.sha256()
    for ln, call in zip(labels, calls):
        seq = []
        for name, _ in call:
            if seq and seq[-1][0] == name:
                seq[-1][1] += 1
            else:
                seq.append([name, 1])
        by_seq.setdefault("  ".join(n + (f" x{c}" if c > 1 else "") for n, c in seq) or "(nothing)", []).append(_case(ln))
        detail.update((ln + " :: " + " ".join(f"{n}@{size}" for n, size in call) + "\n").encode())
    with open(out_path, "w") as out:
        if not ok:
            out.write(f"MISMATCH: {len(labels)} cases, {len(groups)} separators in the trace, {len(cur)} kernels behind the last\n")
        out.write(f"{len(labels)} cases, {len(by_seq)} distinct kernel sequences; per sequence the cases that ran it: mesh, model/parameters, what is\n"
                  "not default of strategy, variant, cluster mode, armed stamps and options, the part, and part=1->n: rows [0, n) complete\n"
                  f"sha256 over every case with the grid / workgroup size / LDS bytes of each launch and what the call reported: {detail.hexdigest()}\n")
        for seq, who in by_seq.items():
            out.write("\n" + seq + "\n")
            on, meshes = {}, {}
            for mesh_model, rest in who:
                on.setdefault(mesh_model, []).append(rest)
            for mesh_model, rest in on.items():                   # meshes on which a model ran the same cases share a line
                mesh, model = mesh_model.split()
                meshes.setdefault((model, "; ".join(rest)), []).append(mesh)
            for (model, rest), ms in meshes.items():
                out.write(textwrap.fill(f"{','.join(ms)} {model}: {rest}", 170, initial_indent="    ", subsequent_indent="        ",
                                        break_long_words=False, break_on_hyphens=False) + "\n")
    print(f"{len(labels)} cases, {len(by_seq)} distinct sequences -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "reduce":
        reduce(*sys.argv[2:])
    else:
        sys.exit(__doc__)
