"""The inputs of tests/test_gpu_rank_rounds.py (tests/rank_census.py) checked on the CPU alone: the conditions that keep the GPU tests
from passing vacuously.  For every leaf form, every named state of k_rank_sorted's rounds, of the staging batches (PF 8 and 4), of the
latch, of the slices and of the split search — and for the Order1 records every round class of k_apm1 — must be reached by at least
one committed input; the inputs are pinned by their sha256, so that these conditions and the GPU run speak of the same bytes.  Run
with -s for the list of which input reaches which state."""
import collections
import hashlib

import numpy as np
import pytest

from tests import rank_census as rc
from tests.synth import markov_text

NAMES = list(rc.SMALL_INPUTS) + [rc.LARGE_INPUT]

SHA256 = {
    "hist_sorted": "6ad769c055d0a1893793c567de1fbc421017314b793f34f4f65b703907bdcd5d",
    "hist_shuffled": "308aeb2ffbbdc082b783113b40815663e9f2ebc673a82fe81906a93f67293233",
    "hist_chunk40": "1be8281f47fd3213d085e993c47a7f8e6c93c1ea660f8238c0747e5edca2e1f4",
    "hist_chunk150": "ff342e1c791261ce666ed7e7d23b0b54ef0ae5cc337d4ffbe235dc7209c543fb",
    "hist_chunk12": "041097018cc0c2637720b39e074d33467017ae3e4e4cb2d527ea1fad49580370",
    "clustered_a": "e8ca9d61bf9f15d3f71aa17a2a13a2ad043898df1c252ad6b4b5acdbd99528c0",
    "clustered_b": "a660be6a9103f45dc27c2478cc3926b3ddf59d134acd1ea5042b4db6e0da7770",
    "batch_head_pf8": "5982b0a419753be91e492a9f1dbfead49a6aa2dea98968bca4da5d537139cb1d",
    "batch_head_pf4": "cfc8e9669eafefb1bdc3c60810f26345e1cc49b9253081cf61e2fe26420bd1eb",
    "latch": "61e3ff27d8690d2618a71a055f432a11744d9934f2a05d42b98a816c0f0a2129",
    "heads_on_ideal": "4236e93a2fb62c7e1d9f419247830e4e6af6595893c1e0f0bab338939c3b26bd",
    "long_last_group": "c68a759ba40de30e7afce01857405c784191603038028b2e424839eb9ad22beb",
    "tiny": "82b39431a0f2b3e96b7e90a553cda42a8285fc9df723ad554c035868114237ac",
    "after_latch": "adf6e89ad3b05fa29923bbf5b04a0fbbd98dbb53f5a4f02abb9f13650b284ea4",
}

# states that only a block of more than 64 * 65400 records can reach (rank_census.after_latch_block)
LARGE_ONLY = {"latch.carried_ends_after", "latch.group_change_after"}


def required(form):
    return rc.RANK_STATES + (rc.APM1_STATES if form == "order1" else [])


def reachers(form):
    """state -> [(input, count)]"""
    out = collections.defaultdict(list)
    for name in NAMES:
        for state, count in rc.block_census(name, form)[0].items():
            out[state].append((name, count))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_pinned(name):
    data = rc.block(name)
    assert len(data) <= (5_000_000 if name == rc.LARGE_INPUT else 70_400 if name == "latch" else 40_000)
    assert hashlib.sha256(data).hexdigest() == SHA256[name], name


@pytest.mark.parametrize("form", rc.FORMS)
def test_every_state_is_reached(form):
    reach = reachers(form)
    print("\n%s" % form)
    for state in required(form):
        print("  %-34s %s" % (state, " ".join("%s(%d)" % r for r in reach.get(state, [])) or "-- no input --"))
    for state in required(form):
        names = [n for n, _ in reach.get(state, [])]
        assert names, "no input reaches %s as a leaf of %s (inputs: %s)" % (state, form, ", ".join(NAMES))
        if state not in LARGE_ONLY:      # everything else has a small input too: the variants and layouts of the GPU tests run on those
            assert [n for n in names if n != rc.LARGE_INPUT], "only %s reaches %s as a leaf of %s" % (rc.LARGE_INPUT, state, form)


@pytest.mark.parametrize("form", rc.FORMS)
def test_the_inputs_built_for_a_state_reach_it(form):
    """what each directed input is there for, by name"""
    def has(name, *states):
        st = rc.block_census(name, form)[0]
        for s in states:
            assert st[s] > 0, "%s does not reach %s as a leaf of %s" % (name, s, form)

    has("batch_head_pf8", "pf8.head_on_batch")
    has("batch_head_pf4", "pf4.head_on_batch")
    has("latch", "latch")
    has(rc.LARGE_INPUT, "latch", "latch.carried_ends_after", "latch.group_change_after")
    has("heads_on_ideal", "split.ideal_on_head")
    assert rc.block_census("heads_on_ideal", form)[0]["split.ideal_on_head"] == 63
    has("long_last_group", "split.walk", "split.shortcut", "split.boundary_is_len")
    has("tiny", "split.block_under_64", "slice.short", "slice.empty")
    has("clustered_a", *rc.ROUND_STATES)      # one block with every round state, in every form


@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_split_invariants(name, form):
    pos, g, c0, ck = rc.records(rc.block(name), form)
    sp = rc.block_census(name, form)[1]
    n = len(g)
    assert np.array_equal(np.sort(pos), np.arange(n))
    assert len(sp) == rc.SLICES + 1 and sp[0] == 0 and sp[rc.SLICES] == n
    assert all(sp[s] <= sp[s + 1] for s in range(rc.SLICES)), "boundaries are not monotone"
    h = rc.head_flags(g)
    for s in range(1, rc.SLICES):
        assert sp[s] == n or h[sp[s]], (s, "the boundary is neither a group head nor the length")
        assert sp[s] >= s * n // rc.SLICES and not h[s * n // rc.SLICES:sp[s]].any(), (s, "not the FIRST head at or after the ideal point")


def test_the_sort_is_stable_and_groups_are_contiguous():
    for form in rc.FORMS:
        pos, g, c0, ck = rc.records(rc.block("hist_chunk40"), form)
        heads = np.flatnonzero(rc.head_flags(g))
        assert len(set(g[heads].tolist())) == len(heads), form            # every group is one run
        inside = ~rc.head_flags(g)
        assert (pos[1:][inside[1:]] > pos[:-1][inside[1:]]).all(), form      # time order inside a group


def test_returned_counts_against_a_serial_replay(monkeypatch):
    """the vectorised count of rank_census._hot against Counter tables kept one record at a time, at a limit small inputs reach"""
    monkeypatch.setattr(rc, "LIM", 40)
    for form in rc.FORMS:
        pos, g, c0, ck = rc.records(rc.block("hist_sorted"), form)
        got = rc._hot(g, c0, ck, 0, len(g))
        want = np.zeros(len(g), dtype=bool)
        tbl, open_g = {}, None
        for t in range(len(g)):
            if g[t] != open_g:
                tbl, open_g = {}, g[t]
            w16 = (int(ck[t]) << 8) | int(c0[t])
            for j in range(8):
                key, bit = (j, (w16 >> (8 - j)) & 0xFF), (int(c0[t]) >> (7 - j)) & 1
                n = tbl.setdefault(key, [0, 0])
                want[t] |= max(n) >= 40
                n[bit] += 1
        assert got.any() and np.array_equal(got, want), form


@pytest.mark.parametrize("form", rc.FORMS)
def test_text_reaches_strictly_fewer_states(form):
    """why the directed inputs exist: the suite's text input, in its blocks of 16 KiB, leaves states of every leaf form unreached"""
    text = rc.census_blocks(markov_text(70000, seed=12), 16384, form)
    reach = reachers(form)
    have_text = {s for s in required(form) if text[s]}
    have_new = {s for s in required(form) if reach.get(s)}
    print("\n%s: text misses %s" % (form, " ".join(sorted(have_new - have_text))))
    assert have_text < have_new, form
