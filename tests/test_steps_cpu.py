"""The per-step statistics export on the CPU (include/w3hip.h "per-step statistics"): w3_steps_layout_of for the model shapes the GPU
tests export, its refusals, and the index arithmetic of the row kernel (weath3rb0i_amd/csrc/w3_steps_plan.h) walked on the host by
tests/host/steps_plan.cpp — every element of every row written exactly once, in both store forms, and the F16 form of every stretch
value against numpy.  No device call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "steps_plan.cpp")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


@pytest.fixture(scope="module")
def lib():
    from weath3rb0i_amd import build
    build.build()
    return L.load()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("steps") / "steps_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    return exe


def _nest(leaves):
    m = leaves[0]
    for nxt in leaves[1:]:
        m = w3.BestOfTwoModel(m, nxt)
    return m


def _leaves(k):
    return [w3.OrderN(8 + i, 3) for i in range(k)]


SHAPES = {   # name -> (model, leaves, APM stages)
    "one_leaf": (lambda: w3.Order0(), 1, 0),
    "three_leaves": (lambda: _nest([w3.Order0(), w3.Order1(), w3.OrderN(27, 3)]), 3, 0),
    "nine_leaves": (lambda: _nest(_leaves(9)), 9, 0),
    "frozen_leaf": (lambda: _nest([w3.Order0(), w3.FrozenModel(w3.Order1())]), 2, 0),
    "one_leaf_apm": (lambda: w3.APM(w3.Order0()), 1, 1),
    "three_leaves_apm": (lambda: w3.APM(_nest([w3.Order0(), w3.Order1(), w3.OrderN(27, 3)])), 3, 1),
    "three_leaves_two_apm": (lambda: w3.APM(w3.APM(_nest([w3.Order0(), w3.Order1(), w3.OrderN(27, 3)])), ctx=L.W3_APM_ORDER1), 3, 2),
    "nine_leaves_two_apm": (lambda: w3.APM(w3.APM(_nest(_leaves(9)))), 9, 2),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("bit", [False, True])
@pytest.mark.parametrize("fmt", ["p_u16", "stretch_i16", "stretch_f16"])
def test_layout_names_the_columns(lib, name, bit, fmt):
    make, n_leaves, n_apm = SHAPES[name]
    lay = w3.Context.steps_layout(make(), fmt, bit)
    want = dict(n_cols=n_leaves + 1 + n_apm + int(bit), n_leaves=n_leaves, col_mix=n_leaves, col_apm0=n_leaves + 1 if n_apm else None,
                n_apm=n_apm, col_final=n_leaves + n_apm, col_bit=n_leaves + 1 + n_apm if bit else None, elem_bytes=2)
    assert lay == want
    # the last model column is the one before the bit column (or the last one)
    assert lay["col_final"] == lay["n_cols"] - 1 - int(bit)


def test_layout_marks_missing_columns_with_uint32_max(lib):
    spec = w3.Order0().spec()
    lay = L.StepsLayout()
    assert lib.w3_steps_layout_of(C.byref(spec), L.W3_STEPS_P_U16, 0, C.byref(lay)) == L.W3_OK
    assert lay.col_apm0 == 0xFFFFFFFF and lay.col_bit == 0xFFFFFFFF and lay.n_cols == 2


def test_layout_refuses_what_it_does_not_know(lib):
    spec = w3.Order0().spec()
    lay = L.StepsLayout()
    for fmt, flags in [(3, 0), (0xFFFF, 0), (0, 2), (0, 3), (2, 0x80000000)]:
        assert lib.w3_steps_layout_of(C.byref(spec), fmt, flags, C.byref(lay)) == L.W3_E_INVALID, (fmt, flags)
    assert lib.w3_steps_layout_of(C.byref(spec), 0, 0, None) == L.W3_E_INVALID
    bad = w3.Order0().spec()
    bad.n_nodes = 0
    assert lib.w3_steps_layout_of(C.byref(bad), 0, 0, C.byref(lay)) == L.W3_E_INVALID
    with pytest.raises(w3.W3Error):
        w3.Context.steps_layout(w3.Order0(), "bf16")
    with pytest.raises(w3.W3Error):
        w3.Context.steps_layout(w3.Order0(), "p_u16", bit=2)


@needs_gxx
@pytest.mark.parametrize("args", [(3, 1, 0, 1), (1, 0, 2, 0), (9, 2, 1, 1)])
def test_the_plan_headers_layout_is_the_librarys(lib, harness, args):
    """steps_layout of the plan header, through the host harness, against the struct the library fills (same header, two compilers)."""
    n_leaves, n_apm, fmt, flags = args
    r = subprocess.run([harness, "layout"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    model = _nest(_leaves(n_leaves))
    for _ in range(n_apm):
        model = w3.APM(model)
    spec = model.spec()
    lay = L.StepsLayout()
    assert lib.w3_steps_layout_of(C.byref(spec), fmt, flags, C.byref(lay)) == L.W3_OK
    assert got == [getattr(lay, k) for k, _ in L.StepsLayout._fields_]


@needs_gxx
@pytest.mark.parametrize("cols", [1, 2, 7, 13])
@pytest.mark.parametrize("n", [8, 63, 64, 65, 4096 + 37, 3 * 1024 + 5])   # one short tile; around one tile; a ragged last tile; a short last block
def test_every_row_element_is_written_once_in_both_store_forms(harness, cols, n):
    r = subprocess.run([harness, "walk", str(cols), str(n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "steps plan ok" in r.stdout, (r.stdout[-200:], r.stderr[-400:])


@needs_gxx
def test_the_harness_catches_a_tile_base_that_ignores_the_columns(harness, tmp_path):
    hdr = os.path.join(ROOT, "weath3rb0i_amd", "csrc", "w3_steps_plan.h")
    src = open(hdr, encoding="utf-8").read()
    old = "{ return tile * W3_STEPS_TILE * C; }"
    assert src.count(old) == 1
    (tmp_path / "mutant.h").write_text(src.replace(old, "{ return tile * W3_STEPS_TILE; }"), encoding="utf-8")
    cpp = open(SRC, encoding="utf-8").read().replace('"../../weath3rb0i_amd/csrc/w3_steps_plan.h"', '"%s"' % (tmp_path / "mutant.h"))
    (tmp_path / "mutant.cpp").write_text(cpp, encoding="utf-8")
    exe = str(tmp_path / "mutant")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, str(tmp_path / "mutant.cpp")])
    r = subprocess.run([exe, "walk", "7", "200"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "FAIL" in r.stderr


@needs_gxx
def test_staged_pieces_are_whole_blocks_and_cover_the_input(harness):
    for n, bs, run in [(4096 + 37, 1024, 2), (4096, 1024, 3), (10, 1024, 2), (5 * 777 + 1, 777, 1)]:
        r = subprocess.run([harness, "pieces", str(n), str(bs), str(run)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        lens = [int(x) for x in r.stdout.split()]
        assert sum(lens) == n and all(x == run * bs for x in lens[:-1]) and 0 < lens[-1] <= run * bs, (n, bs, run, lens)


@needs_gxx
def test_f16_of_every_stretch_value_is_numpys(lib, harness):
    r = subprocess.run([harness, "f16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    pairs = [tuple(int(x) for x in ln.split()) for ln in lines if ln and not ln.startswith("bit")]
    assert [v for v, _ in pairs] == list(range(-2047, 2048))
    v = np.array([p[0] for p in pairs], dtype=np.int32)
    want = (v / 256).astype(np.float16)
    assert (want.astype(np.float64) * 256 == v).all()          # the format holds every value exactly
    assert np.array([p[1] for p in pairs], dtype=np.uint16).tolist() == want.view(np.uint16).tolist()
    bit = [ln for ln in lines if ln.startswith("bit")][0].split()
    assert [int(bit[1]), int(bit[2])] == np.array([0.0, 1.0], dtype=np.float16).view(np.uint16).tolist()
    # the table the STRETCH formats go through stays inside that range
    st = np.zeros(4096, dtype=np.int16)
    sq = np.zeros(4095, dtype=np.uint16)
    assert lib.w3_stretch_squash(st.ctypes.data_as(C.c_void_p), sq.ctypes.data_as(C.c_void_p)) == L.W3_OK
    assert int(st.min()) >= -2047 and int(st.max()) <= 2047
