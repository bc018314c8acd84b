"""The base-weight step on a tree of nested groups without a GPU: the entry points exist, the replay cases of
tests/test_gpu_htree.py sit on no tie and reach the shapes they are there for, the replayed chain keeps the marginals of the
root and of a level-2 row (and two wrong orders do not), the draws depend on (seed, sweep, level, cell) alone, and one level
is the grouped step to the bit."""
import math
import os
import re
from functools import lru_cache

import numpy as np
import pytest

import hh_oracle as hho
import ht_oracle as hto
from libstb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stb_sample_htree", "stb_tindic_set_htree", "stb_tindic_set_htree_level", "stb_tindic_get_htree_level",
         "stb_tindic_sample_htree")
MARGIN = 1e-9        # the Gamma acceptance tests (test_hgroups_host's bars)
MARGIN_Y = 1e-13     # the Bernoulli comparisons, relative
U = 2.0 ** -53


def test_entry_points_exist():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "stb_hip.h")).read()
    source = open(os.path.join(ROOT, "libstb_amd", "capi.py")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert 'sig("%s"' % name in source, name
    for name in ("set_htree", "set_htree_level", "get_htree_level", "sample_htree"):
        assert hasattr(capi.TableIndicators, name), name
    assert hasattr(capi, "sample_htree")
    assert "#define STB_HT_MAXL 8" in header and capi.HT_MAXL == hto.MAXL == 8
    assert (capi.C.sizeof(capi.HTreeOpts), capi.C.sizeof(capi.HTreeInfo)) == (56, 200)
    assert "0x%X" % hto.SALT_L in header.upper().replace("0X", "0x")
    # refused before any device is touched
    _, opts = capi.htree_opts(1, [1.0])
    info = capi.HTreeInfo()
    assert L.stb_sample_htree(3, None, None, 2, None, None, capi.C.byref(opts), None, None, None, None, None, 1, 0, None,
                              capi.C.byref(info)) != 0 and "required" in capi.last_error()
    assert L.stb_tindic_sample_htree(None, capi.C.byref(opts), 1, 0, None) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_set_htree(None, 0, None, None) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_set_htree_level(None, 2, None) != 0 and "null" in capi.last_error()
    assert L.stb_tindic_get_htree_level(None, 1, None) != 0 and "null" in capi.last_error()


@lru_cache(maxsize=None)
def replayed(name, flags):
    return hto.replay_case(name, flags)


@pytest.mark.parametrize("name,flags", hto.STEPS)
def test_replay_cases_sit_on_no_tie(name, flags):
    c, out = hto.case(name, flags), replayed(name, flags)
    print(name, flags, "margins: gamma", out["margin_gamma"], "bernoulli", out["margin_y"], "tables", out["tables"], "aux",
          out["aux_tables"], "alpha'", out["alpha"])
    assert out["margin_gamma"] >= MARGIN and out["margin_y"] >= MARGIN_Y
    L = len(c["G"])
    # no drawn weight underflows (a child's shape alpha * 0 + 0 would be the step's error 4), and every one is large enough
    # for the replay's relative bar
    assert out["min_shape"] >= 0.02 and min(float(r.min()) for r in out["rows"]) > 1e-280 and out["root"].min() > 1e-280
    for l in range(L):
        cl, ml = out["c"][l], out["m"][l]
        assert cl.shape == ml.shape == (c["G"][l], c["Kmax"])
        assert ml.min() >= 0 and np.all(ml <= cl) and np.all((ml >= 1) == (cl >= 1))
        for row in out["rows"][l]:
            assert abs(math.fsum(row) - 1.0) <= 2.0 * U * c["Kmax"]
        if l + 1 < L:      # only the auxiliary tables are handed up
            assert out["tables"][l + 1] == out["aux_tables"][l]
        assert (out["alpha"][l] != c["alpha"][l]) == bool(flags & hto.SAMPLE_ALPHA) and out["alpha"][l] > 0
    assert np.array_equal(out["root"], c["root"]) == bool(flags & hto.KEEP_ROOT)
    # what each case is there for
    if name == "two_ragged":
        assert c["G"] == [7, 3] and len(c["K"]) == 37 and set(np.unique(c["K"])) == {1, 2, 3, 4, 5}
        assert out["c"][0][2].sum() == 0 and c["offs"][0][2] == c["offs"][0][3]          # an empty level-1 range
        assert out["c"][1][1].sum() == 0 and c["offs"][1][1] == c["offs"][1][2]          # a childless level-2 node
    if name == "three_k70":
        assert c["G"] == [9, 4, 2] and c["Kmax"] == 70
        assert out["c"][0].max() > 257 and out["c"][1].max() > 257 and out["c"][1].max() > int(c["t"].max())
        assert out["c"][0][:, 64:].sum() > 0
    if name == "one_each":
        assert c["G"] == [3, 1, 1]
    if name == "few_rows":
        assert c["G"] == [1, 1] and len(c["K"]) == 2 and sorted(out["c"][0][0])[-2:] == [60001, 60001]
        assert out["c"][1].max() > 257
    if name == "k1024":
        assert c["Kmax"] == 1024 and len(c["G"]) == 2
        assert out["c"][0].max() > 257 and (out["c"][0] == 0).any()


@lru_cache(maxsize=None)
def chain(law):
    return hto.law_chain(hto.LAW_SEED, law)


@pytest.mark.parametrize("law", hto.LAWS)
def test_the_replayed_chain_keeps_both_marginals(law):
    kept = chain(law)
    assert len(kept) == hto.LAW_STEPS // hto.LAW_THIN
    p_root, p_node = hto.law_pvalues(kept)
    print(law, "KS p-values: r_0", p_root, "h_A0", p_node, "means", kept.mean(axis=0))
    if law == "right":
        assert p_root > 1e-3 and p_node > 1e-3
    else:
        assert p_node < 1e-9


def test_the_posterior_is_a_distribution():
    post = hto.TreePosterior(points=801)
    for cdf in (post.cdf_r, post.cdf_h):
        assert cdf[0] == 0.0 and cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0)
    # halving the step moves neither CDF by 1e-3: the trapezoid's error falls fourfold a halving, so the fine grid's own is a
    # third of that, some seventy times below the 0.022 = 1 / sqrt(2000) that a KS test of the chain's 2000 values resolves
    fine = hto.TreePosterior(points=1601)
    for a, b in ((post.cdf_r, fine.cdf_r), (post.cdf_h, fine.cdf_h)):
        assert np.abs(a - np.interp(post.x, fine.x, b)).max() < 1e-3


def test_the_draws_depend_on_seed_sweep_level_and_cell_alone():
    c = hto.case("two_ragged")
    args = (c["K"], c["t"], c["offs"], c["root"], c["rows"], c["alpha"], c["gamma"])
    a = hto.replay(*args, 11, 2)
    b = hto.replay(*args, 11, 3)
    d = hto.replay(*args, 12, 2)
    for o in (b, d):
        assert not np.array_equal(a["root"], o["root"]) and np.array_equal(a["c"][0], o["c"][0])
        for l in range(2):
            assert not np.array_equal(a["rows"][l], o["rows"][l])
    # a level's streams are its own: the same counts and weights under the two level keys give other tables
    k1, k2 = hto.level_keys(11, 2, 2)
    assert k1 != k2 and k1 == __import__("hq_oracle").sweep_key(11, 2)
    cc, w = np.full((3, 5), 40), np.full((3, 5), 1.5)
    assert not np.array_equal(hto.aux_tables(cc, w, k1)[0], hto.aux_tables(cc, w, k2)[0])
    # a cell's tables are the same whatever lies around it: the first two rows alone
    assert np.array_equal(hto.aux_tables(cc[:2], w[:2], k2)[0], hto.aux_tables(cc, w, k2)[0][:2])
    # the tree's shape above a level does not reach into the level's tables: level 1's m under another level-2 cut, the
    # level-2 rows being equal
    rows = [None, np.tile(c["rows"][1][0], (3, 1))]
    offs2 = [c["offs"][0], np.array([0, 1, 5, 7], dtype=np.uint64)]
    e = hto.replay(c["K"], c["t"], c["offs"], c["root"], rows, c["alpha"], c["gamma"], 11, 2)
    f = hto.replay(c["K"], c["t"], offs2, c["root"], rows, c["alpha"], c["gamma"], 11, 2)
    assert np.array_equal(e["m"][0], f["m"][0]) and not np.array_equal(e["c"][1], f["c"][1])
    # the pairs hold their level-1 node's row
    assert np.array_equal(a["h"], hho.spread(c["K"], a["owner"], a["rows"][0]))


@pytest.mark.parametrize("name", ["ragged_keep", "ragged_full"])
def test_one_level_is_the_grouped_replay(name):
    c = hho.case(name)
    want = hho.replay_case(name)
    got = hto.replay(c["K"], c["t"], [c["goff"]], c["root"], [None], [c["alpha"]], c["gamma"], c["seed"], c["sweep"], c["flags"],
                     c["shape"], c["scale"], Kmax=c["Kmax"])
    assert np.array_equal(got["c"][0], want["c"]) and np.array_equal(got["m"][0], want["m"])
    assert np.array_equal(got["root"], want["root"]) and got["alpha"][0] == want["alpha"]
    assert np.array_equal(got["rows"][0], want["hgrp"]) and np.array_equal(got["h"], want["h"])
    assert got["margin_gamma"] == want["margin_gamma"] and got["margin_y"] == want["margin_y"]
