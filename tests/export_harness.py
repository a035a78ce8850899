"""What tests/test_export_cpu.py and tests/test_export_entropy_cpu.py share: the blob the case files' inputs are cut from, the build of a
host harness (tests/host/*_lanes.cpp) and the run of one case file through it."""
import os
import re
import subprocess

from tests.synth import lcg_text, markov_text

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(tmp_path_factory, name, src, oracle=None):
    """-> (exe, blob path, directory[, the oracle's object file]): the harness fixture of a module.  The blob is markov_text(300000) |
    lcg_text(300000) | markov_text(70000).  oracle: the directory of w3_oracle.c, for the harness that links it"""
    d = tmp_path_factory.mktemp(name)
    (d / "blob").write_bytes(markov_text(300000) + lcg_text(300000) + markov_text(70000))
    exe = str(d / os.path.splitext(os.path.basename(src))[0])
    if oracle is None:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src])
        return exe, str(d / "blob"), d
    obj = str(d / "w3_oracle.o")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", "-I", oracle, "-o", obj, os.path.join(oracle, "w3_oracle.c")])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", oracle, "-o", exe, src, obj, "-lpthread", "-lm"])
    return exe, str(d / "blob"), d, obj


def sanitizer_probe(tmp_path):
    """-> the empty string if g++ links the sanitizer runtime, else why it does not"""
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(tmp_path / "probe.cpp")], capture_output=True, text=True)
    return "" if r.returncode == 0 else "g++ cannot link the sanitizer runtime: " + r.stderr[-200:]


def answers(harness, cases, name, exe=None, text=("fold",)):
    """the cases through the harness: every answer line must be "ok k=v ..." -> one dict per case (the values of `text` stay strings)"""
    exe0, blob_path, d = harness[:3]
    p = d / name
    p.write_text("\n".join(cases) + "\n")
    r = subprocess.run([exe or exe0, blob_path, str(p)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-800:])   # (-11: a read outside the buffer)
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    bad = [(c, ln[:200]) for c, ln in zip(cases, lines) if not ln.startswith("ok")]
    assert not bad, bad[:5]
    return [{k: (v if k in text else int(v)) for k, v in re.findall(r"(\w+)=(\S+)", ln)} for ln in lines]
