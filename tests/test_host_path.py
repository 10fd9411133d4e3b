"""Which kernel runs (rdcfes_amd/csrc/rdc_path.h; DESIGN.md, "Which kernel runs"): the decision function through the host shim,
as a table of (model, facts) -> (kernel family, instantiation, two-part mode).

The expected values are what the commit before the decision function ran, read off its kernel trace: every row of the table is a
case of profiles/path_matrix_parent.txt (tools/path_matrix.py: the same mesh, model, parameters, options and part), and states
the kernel that file lists the case under.  A launch of nothing in part 1 followed by everything in part 2 is ALL_IN_PART2.
The list facts of the rows come from real lists (the mesh named in the row, built here as the context builds them at the
upload and on the first assembly), the rest of the facts from the row."""
import ctypes as C

import pytest

import meshes
from rdcfes_amd import partition, synth

PATHS = ["TET4_CL", "TET4_EV", "TET4_EVC", "TET4_RG5", "TET4_RG3", "TET4_RG2", "TET4_ROWGATHER", "TET4_COLOURED", "HEX8_CL",
         "HEX8_CL_ROWS", "GENERIC_ROWGATHER", "GENERIC_COLOURED"]
INSTS = ["FULL", "SPARSE", "MOMENTS"]
TWO_PART = ["WHOLE", "EV_SPLIT", "CL_SPLIT", "PAIR_SPLIT", "ALL_IN_PART2"]
MODEL = {"pihna": 0, "ripf": 1, "hcc": 2, "adpm": 4, "proteas": 5}
NV = {"pihna": 5, "ripf": 3, "hcc": 3, "adpm": 3, "proteas": 5}
AUTO, COLOURED, ROWGATHER = 0, 1, 2            # RDC_SCATTER_*
GENERIC = 1                                    # RDC_VARIANT_GENERIC
MAX_LDS = 160 * 1024                           # of the device the trace was taken on
FACTS = ["nen", "strategy", "variant", "tet4_cl_mode", "pattern", "stamps", "rowgather_ok", "rg2_ok", "rg2_block", "pair_aux", "nlist",
         "pair_eid", "ev_ok", "ev_tried", "cl_ready", "cl_fits"]


def _mesh(name):
    """(nen, conn, n_node, n_owned) of the meshes of tools/path_matrix.py, and the Delaunay mesh of test_host_highvalence.py"""
    if name == "ghost":            # the ghosted K(8) partition of tests/test_host_parts.py
        conn, xyz = synth.kuhn_tet_mesh(8, order="random")
        lp = partition.build_local(conn, xyz, partition.partition_rcb(xyz[conn].mean(axis=1), 3), 1, 3)
        return 4, lp.conn, lp.xyz.shape[0], lp.n_owned
    if name == "hydrogel":
        conn, xyz = meshes.hydrogel()
    elif name == "delaunay":
        from test_host_highvalence import delaunay_tets
        conn, xyz = delaunay_tets()
    elif name == "H5":
        conn, xyz = synth.hex_mesh(5, jitter=0.15, order="random")
        return 8, conn, xyz.shape[0], xyz.shape[0]
    else:                          # K7, K9, K12
        conn, xyz = synth.kuhn_tet_mesh(int(name[1:]), order="random" if name == "K7" else "lex")
    return 4, conn, xyz.shape[0], xyz.shape[0]


def decide(shim, model, facts, opts):
    keys = (C.c_char_p * len(opts))(*[k.encode() for k in opts])
    vals = (C.c_int * len(opts))(*opts.values())
    out = (C.c_int * 8)()
    assert shim.shim_path_decide(MODEL[model], (C.c_int * 16)(*[int(facts[k]) for k in FACTS]), len(opts), keys, vals, out) == 0
    return {"path": PATHS[out[0]], "inst": INSTS[out[1]], "two_part": TWO_PART[out[2]], "ev_general": bool(out[3]),
            "builds": {"ev": bool(out[4]), "tet4_cl": bool(out[5]), "hex8_cl": bool(out[6]), "pair_eid": bool(out[7])}}


def plan_on_mesh(shim, make_prep, mesh, model, pattern, opts=None, strategy=AUTO, variant=0, cl_mode=0, stamps=False, cl_lds=MAX_LDS,
                 ev_from_before=False):
    """The plan of an assembly call on a fresh context holding `mesh`: the lists of the upload, the builds the decision asks
    for, then the decision.  ev_from_before: a three-unknown context whose element-visit lists an earlier call built."""
    opts = dict(opts or {})
    nen, conn, n_node, n_owned = _mesh(mesh)
    nv = NV[model]
    if opts.get("part"):
        opts.setdefault("interior_nodes", int(0.6 * n_owned))
    P = make_prep(nen, conn, n_node, n_owned, nv, lds_budget=meshes.LDS_BUDGET, block=opts.get("block", 256))
    assert P.ok, P.error
    st = (C.c_int64 * 6)()

    def ev_build():
        shim.shim_ev_build_interior.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        return shim.shim_ev_build_interior(54000, -1, st) == 0

    ev = nen == 4 and (nv == 5 or ev_from_before) and P.rg2_ok and ev_build()         # rdc_mesh_upload
    lf = (C.c_int * 16)()
    shim.shim_path_list_facts(int(ev), lf)
    facts = dict(zip(FACTS, lf))
    rg = facts["rowgather_ok"] or (facts["rg2_ok"] and variant != GENERIC)            # resolve_strategy
    facts.update(strategy=(ROWGATHER if rg else COLOURED) if strategy == AUTO else strategy, variant=variant, tet4_cl_mode=cl_mode,
                 pattern=pattern, stamps=stamps, ev_tried=nen == 4 and (nv == 5 or ev_from_before) and P.rg2_ok)
    builds = decide(shim, model, facts, opts)["builds"]
    if builds["ev"]:
        facts.update(ev_ok=ev_build(), ev_tried=True)
    if builds["tet4_cl"]:
        out = (C.c_int64 * 2)()
        shim.shim_path_build_tet4_cl(out)
        facts.update(cl_ready=bool(out[0]), cl_fits=bool(out[0]) and out[1] <= cl_lds)
    if builds["hex8_cl"]:
        facts.update(cl_ready=True)          # the HEX8 lists of these meshes build (tests/test_host_cl.py)
    return decide(shim, model, facts, opts), facts


# (mesh, model, pattern applies, call, expected path, instantiation or None where the family
# has one form only, two-part mode); call = options plus strategy / variant / cl_mode / stamps.  PIHNA "shipped", RIPF / HCC / ADPM
# "shipped" are the parameter sets whose pattern applies.
S, G = {"strategy": COLOURED}, {"variant": GENERIC}
TABLE = [
    # PIHNA on a Kuhn mesh: strategy, variant, every knob that leaves the element-visit kernel
    ("K9", "pihna", True, {}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, G, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("K9", "pihna", True, S, "TET4_COLOURED", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {**S, **G}, "GENERIC_COLOURED", "FULL", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 1}, "TET4_ROWGATHER", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 2}, "TET4_RG2", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 3}, "TET4_RG3", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 5}, "TET4_RG5", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 7}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, {"ablate": 1}, "TET4_RG5", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"kernel": 7, "ablate": 4}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, {"lds_pad": 8}, "TET4_RG5", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"ev_general": 0}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, {"ev_general": 0, "specialise": 0}, "TET4_RG5", "FULL", "WHOLE"),
    ("K9", "pihna", True, {"block": 128}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, {"block": 128, "kernel": 3}, "TET4_RG3", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"occupancy": 1}, "TET4_RG5", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"specialise": 0}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", True, {"moments": 0}, "TET4_RG5", "SPARSE", "WHOLE"),
    ("K9", "pihna", True, {"stamps": True}, "TET4_RG5", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"stamps": True, "kernel": 3}, "TET4_RG3", "MOMENTS", "WHOLE"),
    ("K9", "pihna", True, {"stamps": True, "kernel": 7, "ablate": 4}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", False, {}, "TET4_EV", None, "WHOLE"),
    ("K9", "pihna", False, S, "TET4_COLOURED", "FULL", "WHOLE"),
    ("K9", "pihna", False, {"kernel": 3}, "TET4_RG3", "FULL", "WHOLE"),
    ("K9", "pihna", False, {"ev_general": 0}, "TET4_RG5", "FULL", "WHOLE"),
    # ... in two parts: each split mode and a path without sub-ranges
    ("K12", "pihna", True, {"part": 1}, "TET4_EV", None, "EV_SPLIT"),
    ("K12", "pihna", True, {"part": 2}, "TET4_EV", None, "EV_SPLIT"),
    ("ghost", "pihna", True, {"part": 1}, "TET4_EV", None, "EV_SPLIT"),
    ("K12", "pihna", True, {"part": 1, "kernel": 3}, "TET4_RG3", "MOMENTS", "ALL_IN_PART2"),
    ("K12", "pihna", True, {"part": 2, "kernel": 3}, "TET4_RG3", "MOMENTS", "ALL_IN_PART2"),
    ("K12", "pihna", True, {"part": 1, "kernel": 5}, "TET4_RG5", "MOMENTS", "PAIR_SPLIT"),
    ("K12", "pihna", True, {"part": 2, "kernel": 5}, "TET4_RG5", "MOMENTS", "PAIR_SPLIT"),
    ("K12", "pihna", True, {"part": 1, "occupancy": 1}, "TET4_RG5", "MOMENTS", "PAIR_SPLIT"),
    ("K12", "pihna", True, {"part": 1, "moments": 0}, "TET4_RG5", "SPARSE", "PAIR_SPLIT"),
    # the three-unknown models and the models that exist as k_tet4_rg5 and k_tet4_coloured only
    ("K9", "ripf", True, {}, "TET4_RG5", "SPARSE", "WHOLE"),
    ("K9", "ripf", True, S, "TET4_COLOURED", "SPARSE", "WHOLE"),
    ("K9", "ripf", True, {"kernel": 3}, "TET4_RG3", "SPARSE", "WHOLE"),
    ("K12", "ripf", True, {"part": 1}, "TET4_RG5", "SPARSE", "PAIR_SPLIT"),
    ("K9", "ripf", False, {}, "TET4_EVC", "FULL", "WHOLE"),
    ("K12", "ripf", False, {"part": 1}, "TET4_EVC", "FULL", "EV_SPLIT"),
    ("K9", "ripf", False, {"kernel": 3}, "TET4_RG3", "FULL", "WHOLE"),
    ("K9", "ripf", False, {"kernel": 7}, "TET4_RG5", "FULL", "WHOLE"),
    ("K12", "ripf", False, {"part": 1, "kernel": 7}, "TET4_RG5", "FULL", "PAIR_SPLIT"),
    ("K9", "hcc", True, {}, "TET4_RG5", "SPARSE", "WHOLE"),
    ("K9", "hcc", False, {}, "TET4_RG5", "FULL", "WHOLE"),
    ("K12", "hcc", False, {"part": 1}, "TET4_RG5", "FULL", "PAIR_SPLIT"),
    ("K9", "adpm", True, {}, "TET4_RG5", "SPARSE", "WHOLE"),
    ("K9", "adpm", True, {"kernel": 3}, "TET4_RG3", "SPARSE", "WHOLE"),
    ("K12", "adpm", True, {"part": 1}, "TET4_RG5", "SPARSE", "PAIR_SPLIT"),
    ("K9", "adpm", False, {}, "TET4_RG5", "FULL", "WHOLE"),
    ("K9", "adpm", False, S, "TET4_COLOURED", "FULL", "WHOLE"),
    ("K9", "adpm", False, {"kernel": 3}, "TET4_RG5", "FULL", "WHOLE"),
    ("K12", "adpm", False, {"part": 1, "kernel": 3}, "TET4_RG5", "FULL", "ALL_IN_PART2"),      # the quirk: rg5, unsplit
    ("K9", "proteas", False, {}, "TET4_RG5", "FULL", "WHOLE"),
    ("K9", "proteas", False, S, "TET4_COLOURED", "FULL", "WHOLE"),
    ("K12", "proteas", False, {"part": 1, "kernel": 3}, "TET4_RG5", "FULL", "ALL_IN_PART2"),
    # HEX8: "hex_kernel", "solid_cl_waves", "part" with "hex_kernel"
    ("H5", "pihna", True, {}, "HEX8_CL_ROWS", "FULL", "WHOLE"),
    ("H5", "pihna", True, S, "GENERIC_COLOURED", "FULL", "WHOLE"),
    ("H5", "pihna", True, {"part": 1}, "HEX8_CL_ROWS", "FULL", "CL_SPLIT"),
    ("H5", "pihna", True, {"part": 2}, "HEX8_CL_ROWS", "FULL", "CL_SPLIT"),
    ("H5", "pihna", True, {"hex_kernel": 1}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("H5", "pihna", True, {"hex_kernel": 2}, "HEX8_CL_ROWS", "FULL", "WHOLE"),
    ("H5", "pihna", True, {"hex_kernel": 2, "part": 1}, "GENERIC_ROWGATHER", "FULL", "ALL_IN_PART2"),
    ("H5", "pihna", True, {"solid_cl_waves": 62}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("H5", "hcc", True, {}, "HEX8_CL", "SPARSE", "WHOLE"),
    ("H5", "hcc", True, S, "GENERIC_COLOURED", "SPARSE", "WHOLE"),
    ("H5", "hcc", True, {"hex_kernel": 1}, "GENERIC_ROWGATHER", "SPARSE", "WHOLE"),
    ("H5", "adpm", False, {}, "HEX8_CL", "FULL", "WHOLE"),
    ("H5", "hcc", False, {"hex_kernel": 1, "part": 1}, "GENERIC_ROWGATHER", "FULL", "ALL_IN_PART2"),
    # a mesh without pair lists, and rdc_tet4_cluster_mode 0, 1, 2 with and without them
    ("hydrogel", "pihna", True, {}, "TET4_ROWGATHER", "MOMENTS", "WHOLE"),
    ("hydrogel", "pihna", True, {"part": 1}, "TET4_ROWGATHER", "MOMENTS", "ALL_IN_PART2"),
    ("hydrogel", "pihna", True, G, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("hydrogel", "adpm", False, {}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("hydrogel", "adpm", False, S, "TET4_COLOURED", "FULL", "WHOLE"),
    ("hydrogel", "proteas", False, {}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 1}, "TET4_CL", "MOMENTS", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 1, "part": 1}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("hydrogel", "pihna", True, {"cl_mode": 1, "part": 2}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("hydrogel", "pihna", True, {"cl_mode": 2}, "TET4_CL", "MOMENTS", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 2, "part": 1}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("hydrogel", "pihna", True, {"cl_mode": 2, "part": 2}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("hydrogel", "pihna", True, {"cl_mode": 2, **S}, "TET4_COLOURED", "MOMENTS", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 2, **G}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 1, **S}, "TET4_COLOURED", "MOMENTS", "WHOLE"),
    ("hydrogel", "pihna", True, {"cl_mode": 1, **G}, "GENERIC_ROWGATHER", "FULL", "WHOLE"),
    ("hydrogel", "adpm", False, {"cl_mode": 1}, "TET4_CL", "FULL", "WHOLE"),
    ("hydrogel", "proteas", False, {"cl_mode": 1}, "TET4_CL", "FULL", "WHOLE"),
    ("K7", "pihna", True, {"cl_mode": 1, "part": 1}, "TET4_EV", None, "EV_SPLIT"),
    ("K7", "pihna", True, {"cl_mode": 2, "part": 1}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("ghost", "pihna", True, {"cl_mode": 2, "part": 1}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("ghost", "pihna", True, {"cl_mode": 2, "part": 2}, "TET4_CL", "MOMENTS", "CL_SPLIT"),
    ("K7", "pihna", True, {"cl_mode": 2}, "TET4_CL", "MOMENTS", "WHOLE"),
    ("K7", "ripf", True, {"cl_mode": 2, "part": 1}, "TET4_CL", "SPARSE", "CL_SPLIT"),
    ("K7", "ripf", False, {"cl_mode": 2, "part": 1}, "TET4_CL", "FULL", "CL_SPLIT"),
]
CALL_KEYS = ("strategy", "variant", "cl_mode", "stamps")


def _run_row(shim, make_prep, mesh, model, pattern, call, **kw):
    opts = {k: v for k, v in call.items() if k not in CALL_KEYS}
    return plan_on_mesh(shim, make_prep, mesh, model, pattern, opts, **{k: v for k, v in call.items() if k in CALL_KEYS}, **kw)


def _id(r):
    return "-".join([r[0], r[1], "shipped" if r[2] else "full"] + [f"{k}={int(v)}" for k, v in r[3].items()])


@pytest.mark.parametrize("mesh,model,pattern,call,path,inst,two_part", TABLE, ids=[_id(r) for r in TABLE])
def test_the_plan_is_what_the_parent_ran(shim, make_prep, mesh, model, pattern, call, path, inst, two_part):
    plan, facts = _run_row(shim, make_prep, mesh, model, pattern, call)
    assert (plan["path"], plan["two_part"]) == (path, two_part), (plan, facts)
    if inst is not None:
        assert plan["inst"] == inst, (plan, facts)
    if path == "TET4_EV":                   # k_tet4_ev<.., false> on the shipped pattern with "specialise", <.., true> otherwise
        assert plan["ev_general"] == (not (pattern and call.get("specialise", 1))), plan


def test_every_value_of_the_enums_is_in_the_table():
    assert {r[4] for r in TABLE} == set(PATHS)
    assert {r[5] for r in TABLE} - {None} == set(INSTS)
    assert {r[6] for r in TABLE} == set(TWO_PART)


def test_an_image_beyond_the_lds_leaves_the_call_on_its_path(shim, make_prep):
    """No device in the trace has less LDS than the image of k_tet4_cl needs, so this row states the rule of the parent's
    assemble_rd instead ("a refused build or an image beyond the device's LDS leaves the call on the path it would have
    taken"): hydrogel in mode 1 then runs what it runs in mode 0 (the hydrogel rows of the table)."""
    for call, two_part in (({"cl_mode": 1}, "WHOLE"), ({"cl_mode": 1, "part": 1}, "ALL_IN_PART2")):
        plan, facts = _run_row(shim, make_prep, "hydrogel", "pihna", True, call, cl_lds=16 * 1024)
        assert facts["cl_ready"] and not facts["cl_fits"]
        assert (plan["path"], plan["inst"], plan["two_part"]) == ("TET4_ROWGATHER", "MOMENTS", two_part)


def test_ripf_keeps_the_element_visit_split_of_lists_an_earlier_call_built(shim, make_prep):
    """The quirk of DESIGN.md: "kernel" = 7 on a context whose element-visit lists exist runs k_tet4_rg5 on the whole mesh in both
    parts but reports the element-visit bound.  (A fresh context never builds the lists for "kernel" = 7: the K12 ripf row with "kernel" = 7 of the table.)"""
    plan, _ = _run_row(shim, make_prep, "K12", "ripf", False, {"kernel": 7, "part": 1}, ev_from_before=True)
    assert (plan["path"], plan["inst"], plan["two_part"]) == ("TET4_RG5", "FULL", "EV_SPLIT")


@pytest.mark.parametrize("opts,two_part", [({}, "EV_SPLIT"), ({"kernel": 7}, "EV_SPLIT"), ({"kernel": 5}, "PAIR_SPLIT"),
                                           ({"moments": 0}, "PAIR_SPLIT"), ({"occupancy": 1}, "PAIR_SPLIT"),
                                           ({"kernel": 1}, "ALL_IN_PART2"), ({"kernel": 3}, "ALL_IN_PART2")])
def test_the_prediction_facts_of_part1_nodes(shim, make_prep, opts, two_part):
    """rdc_part1_nodes before the first part-1 call decides for a shipped-pattern PIHNA call, part 1, on the lists that exist: the
    split the part-1 call of the K12 pihna/shipped case with these options then used (the rows that case completed: 1318 = the
    element-visit bound, 1310 = the pair bound, or none)."""
    plan, _ = plan_on_mesh(shim, make_prep, "K12", "pihna", True, {**opts, "part": 1})
    assert plan["two_part"] == two_part


def test_list_facts_of_the_real_meshes(shim, make_prep):
    """what the rows above rest on: Kuhn meshes and the ghosted partition have every list, the hydrogel mesh and the Delaunay
    mesh (rows of more than 16 node blocks) only the row gather"""
    for mesh, has in (("K9", True), ("K12", True), ("ghost", True), ("hydrogel", False), ("delaunay", False)):
        _, facts = plan_on_mesh(shim, make_prep, mesh, "pihna", True)
        assert facts["nen"] == 4 and facts["rowgather_ok"]
        assert [bool(facts[k]) for k in ("rg2_ok", "pair_aux", "nlist", "pair_eid", "ev_ok")] == [has] * 5, (mesh, facts)
