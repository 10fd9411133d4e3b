"""The decision of rdcfes_amd/csrc/rdc_const_rows.h -- may a PIHNA element-visit launch leave the a rows of the value array as an
earlier launch wrote them -- on the CPU: tests/host_const_rows_main.cpp drives the record through every transition the launch code
makes (first launch, key changes, uptake on, mesh upload, coordinate update, another kernel path, a failed launch, the two parts
and a changed split, pointer hand-outs under "const_rows" 0 / 1 / 2, captured launches) and asserts the rows to write after each.
Built as a stand-alone program with AddressSanitizer and UBSan, and run."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_every_transition_of_the_record():
    out = ROOT / "tests" / "_build" / "host_const_rows_asan"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_const_rows_main.cpp"
    deps = [src, ROOT / "rdcfes_amd" / "csrc" / "rdc_const_rows.h"]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", str(src), "-o", str(out)], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and not r.stderr
