"""include/rdc_marshal.h on the CPU: the one place where reference parameter keys become C-ABI struct fields, where the solid
system's material table and side list are built, and where the pipelined hand-back is scheduled -- shared by the libMesh adapter
(integration/libmesh_adapter.C, not compiled here) and the host mirror (rdcfes_amd/host/rdc_host.h).  A stand-alone program
(tests/host_marshal_main.cpp, linked with the fake of tests/fake_rdc_handback.cpp instead of the library) instantiates it with the
mirror's Parameters and with a second, minimal store; its output is compared with rdcfes_amd/params.py and with literals."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import pytest

from rdcfes_amd import params as P
from rdcfes_amd import synth

ROOT = Path(__file__).resolve().parent.parent
STORES = ["mirror", "minimal"]

# struct -> (ctypes mirror, reference key -> (field, index or None))
_flat = lambda keys: {k: (f, None) for k, f in keys.items()}
STRUCTS = {
    "pihna": (P.PihnaParams, _flat(P.PIHNA_KEYS)), "ripf": (P.RipfParams, _flat(P.RIPF_KEYS)), "hcc": (P.HccParams, _flat(P.HCC_KEYS)),
    "adpm": (P.AdpmParams, P.ADPM_KEYS), "proteas": (P.ProteasParams, _flat(P.PROTEAS_KEYS)),
    "pihna_ranges": (P.PihnaRanges, _flat(P.PIHNA_RANGES_KEYS)), "ripf_ranges": (P.RipfRanges, _flat(P.RIPF_RANGES_KEYS)),
}


@pytest.fixture(scope="module")
def prog():
    out = ROOT / "tests" / "_build" / "host_marshal_main"
    out.parent.mkdir(exist_ok=True)
    srcs = [ROOT / "tests" / "host_marshal_main.cpp", ROOT / "tests" / "fake_rdc_handback.cpp"]
    deps = srcs + [ROOT / "include" / "rdc_marshal.h", ROOT / "include" / "rdc_assembly.h", ROOT / "rdcfes_amd" / "host" / "rdc_host.h"]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *map(str, srcs), "-o", str(out)], check=True)
    return out


def _run(prog, *args):
    return subprocess.run([str(prog), *map(str, args)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def tables(prog):
    r = _run(prog, "tables")
    assert r.returncode == 0, r.stderr
    t = {}
    for line in r.stdout.splitlines():
        name, key, offset, kind = line.split()
        assert key not in t.setdefault(name, {}), f"{name}: {key} listed twice"
        t[name][key] = (int(offset), kind)
    return t


def test_every_struct_has_a_table(tables):
    assert set(tables) == set(STRUCTS)


@pytest.mark.parametrize("name", list(STRUCTS))
def test_key_table_against_python(tables, name):
    cls, keys = STRUCTS[name]
    assert set(tables[name]) == set(keys)
    for key, (field, idx) in keys.items():
        offset = getattr(cls, field).offset + (0 if idx is None else idx * C.sizeof(C.c_double))
        assert tables[name][key][0] == offset, key
    assert {k for k, (_, kind) in tables[name].items() if kind == "int"} == ({"RT_dose/total/max"} if name == "ripf" else set())
    # the table covers the struct: every byte but "time" (an argument) and the explicit padding belongs to one key
    covered = sum(4 if kind == "int" else 8 for _, kind in tables[name].values())
    assert covered == C.sizeof(cls) - {"adpm": 8, "ripf": 4}.get(name, 0)


def _case(name):
    """(reference-keyed dict as es.parameters holds it, the struct params.py makes of it)"""
    if name == "pihna":
        d = synth.pihna_param_dict("full")
        return {**P.PIHNA_DEFAULTS, **d}, P.pihna_params_from_dict(d)
    if name == "ripf":
        d = {**synth.ripf_param_dict("full"), "volume_fraction/max_vacant": 0.5}
        return {**P.RIPF_DEFAULTS, **d}, P.ripf_params_from_dict(d)
    if name == "hcc":
        d = synth.hcc_param_dict("full")
        return {**P.HCC_DEFAULTS, **d}, P.hcc_params_from_dict(d)
    if name == "adpm":
        d = {**P.ADPM_DEFAULTS, **synth.adpm_param_dict("full")}
        d["taxis/A_b/angle"] = math.radians(d["taxis/A_b/angle"])      # es.parameters holds radians (src/adpm.C:193)
        d["taxis/Tau/angle"] = math.radians(d["taxis/Tau/angle"])
        d["time"] = 3.0
        return d, P.adpm_params_from_dict(synth.adpm_param_dict("full"), time=3.0)
    if name == "proteas":
        d = synth.proteas_param_dict("full")
        return {**P.PROTEAS_DEFAULTS, **d}, P.proteas_params_from_dict(d)
    if name == "pihna_ranges":
        v = (100.0, 1e9, 50.0, 1e9, 0.0, 7000.0, 0.031, 1.0, 2.39e5)
        return dict(zip(P.PIHNA_RANGES_KEYS, v)), P.PihnaRanges(*v)
    v = (-1e9, 1e9, 0.25, -900.0, 1e9, 0.125)
    return dict(zip(P.RIPF_RANGES_KEYS, v)), P.RipfRanges(*v)


def _write(path, d):
    path.write_text("".join(f"{k} {v!r}\n" for k, v in d.items()))
    return path


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("name", list(STRUCTS))
def test_struct_bytes_against_python(prog, tmp_path, name, store):
    d, expected = _case(name)
    r = _run(prog, "read", store, name, _write(tmp_path / "params.txt", d), tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bin").read_bytes() == bytes(expected)
    if name == "ripf":
        assert bytes(expected)[-4:] == b"\0\0\0\0"        # _pad


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("name,key", [("pihna", "time_step"), ("pihna", "decay/a"), ("adpm", "transform/Tau/trapezoid/2"),
                                      ("ripf", "RT_dose/total/max")])
def test_missing_key_is_named(prog, tables, tmp_path, name, key, store):
    d, _ = _case(name)
    assert list(tables["pihna"])[0] == "time_step" and list(tables["pihna"])[-1] == "decay/a"     # the first and the last key read
    del d[key]
    r = _run(prog, "read", store, name, _write(tmp_path / "params.txt", d), tmp_path / "out.bin")
    assert r.returncode == 1 and f"'{key}'" in r.stderr, r.stderr


@pytest.mark.parametrize("store", STORES)
def test_material_table_and_side_list(prog, tmp_path, store):
    material = lambda i: [1000.0 + i, 0.25 + i / 100.0, 10.0 * i, i + 0.1, i + 0.2, i + 0.3]
    disp = {2: (0.5, float("nan"), -2.0), 5: (0.0, 1.25, float("nan")), 8: (9.0, 9.0, 9.0)}
    sides = [(4, 1, 5), (0, 3, 2), (5, 0, 2), (2, 2, 8)]                        # (elem, side, id)
    lines = ["pseudo_time 0.375", "BCs/displacement_penalty 100000.0", "bool solver/assembly_use_symmetry 1", "string BCs 2 5",
             "subdomains 7 3 7 9 3 3"]
    for i in (3, 7, 9, 4):                                                       # 4: a material no element has
        names = ["Young", "Poisson", "FibreStiffness"] + [f"VolumetricStretchRatio/rate_{d}" for d in range(3)]
        lines += [f"material/{i}/Hyperelastic/{n} {v!r}" for n, v in zip(names, material(i))]
    lines += [f"point BC/{i}/displacement {u[0]!r} {u[1]!r} {u[2]!r}" for i, u in disp.items()]
    lines += [f"side {e} {s} {i}" for e, s, i in sides]
    (tmp_path / "solid.txt").write_text("\n".join(lines) + "\n")
    r = _run(prog, "solid", store, tmp_path / "solid.txt")
    assert r.returncode == 0, r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    assert [l for l in out if l[0] == "params"] == [["params", "0.375", "100000", "1", "0"]]
    assert [l[1:] for l in out if l[0] == "elem_material"] == [["0", "1", "0", "2", "1", "1"]]
    assert [[float(x) for x in l[1:]] for l in out if l[0] == "material"] == [material(7), material(3), material(9)]   # first seen first
    got = [(int(l[1]), int(l[2]), tuple(float(x) for x in l[3:])) for l in out if l[0] == "side"]
    want = [(0, 3, disp[2]), (5, 0, disp[2]), (4, 1, disp[5])]                   # ascending id, then input order; id 8 is not in "BCs"
    assert len(got) == 3 and [g[:2] for g in got] == [w[:2] for w in want]
    for g, w in zip(got, want):
        assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(g[2], w[2]))


def _handback_passes(stdout):
    """the program's log, cut at its "# handback" / "# release" marks: [(mark words, [call words])]"""
    passes = []
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "#" and w[1] in ("handback", "release", "reallocated"):
            passes.append((w[1:], []))
        else:
            passes[-1][1].append(w)
    return passes


@pytest.mark.parametrize("n_nodes,n_chunks", [(27, 1), (27, 2), (27, 7), (5, 40)])
def test_handback_schedule(prog, n_nodes, n_chunks):
    r = _run(prog, "handback", n_nodes, n_chunks)
    assert r.returncode == 0, r.stderr
    passes = _handback_passes(r.stdout)
    assert [m[0] for m, _ in passes] == ["handback", "handback", "release", "handback", "reallocated", "handback", "handback", "release"]
    for (mark, calls), complete in zip([p for p in passes if p[0][0] == "handback"], [True, True, True, True, False]):
        outstanding, ranges, consumed, waited = {}, {}, [], set()
        for w in calls:
            if w[0] == "async":
                outstanding[int(w[3])] = ranges[int(w[3])] = (int(w[1]), int(w[2]))
                assert len(outstanding) <= 2                                      # never more than two tickets in flight
            elif w[0] == "wait":
                waited.add(outstanding.pop(int(w[1])))
            elif w[0] == "consume":
                assert (int(w[1]), int(w[2])) in waited and w[3] == "ok"          # not before its wait; its rows are there
                consumed.append((int(w[1]), int(w[2])))
        if not complete:                                                          # the injected failure: one error, with the call's name
            assert ["#", "error", "rdc_ticket_wait:", "fake", "failure", "of", "rdc_ticket_wait"] in calls and not consumed
            continue
        assert len(consumed) == n_chunks and consumed[0][0] == 0 and consumed[-1][1] == n_nodes
        assert all(a[1] == b[0] for a, b in zip(consumed, consumed[1:])) and all(a <= b for a, b in consumed)   # a partition, in order
        assert n_nodes >= n_chunks or any(a == b for a, b in consumed)           # (5, 40): the empty ranges are delivered too
        assert ["#", "equal", "1"] in calls                                       # the destination equals the source
    count = lambda calls, what: sum(w[0] == what for w in calls)
    first, second, release, third, _, fourth, fifth, last = [calls for _, calls in passes]
    assert count(first, "pin") == 2 and count(second, "pin") == 0                 # two hand-backs on the same arrays: two pins, not four
    assert count(first + second, "unpin") == 0 and [w[0] for w in release] == ["unpin", "unpin"]     # unpinned at release only
    assert {w[1] for w in release} == {w[1] for w in first if w[0] == "pin"}
    assert count(third, "pin") == 2 and count(third, "unpin") == 0                # released: the next hand-back pins again
    val4, rhs4 = passes[5][0][3], passes[5][0][5]
    assert val4 != passes[3][0][3] and rhs4 == passes[3][0][5]                    # val moved, rhs did not ...
    assert [w[:2] for w in fourth if w[0] in ("pin", "unpin")][-2:] == [["pin", val4], ["pin", rhs4]]   # ... and both are pinned where they are now
    assert count(fifth, "pin") == 0 and sorted(w[1] for w in last) == sorted([val4, rhs4])
