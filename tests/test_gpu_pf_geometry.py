"""k_seat_pf (libstb_amd/csrc/seat_pf.hip) past one restaurant a workgroup: a launch of 2 * 2^20 + 8 restaurants, in which
workgroups 0 to 7 of the capped grid take three restaurants each, one after the other (tests/pf_oracle.py, chain_case; every
other restaurant has no dishes and no customers).  What a workgroup hands from one restaurant to the next -- its
registers, the two LDS buffers laid out by the predecessor's K, the barrier count of waves that left a restaurant early --
must not reach the results:

  1. the listed restaurants of the full launch bit for bit against the numpy replay, and against a launch of the listed
     restaurants alone, where each has a workgroup of its own; H_i within the bar of pf_oracle's docstring;
  2. the fillers on the device: H_i = 0, w = 1, E = 0, res = 0, nothing counted;
  3. the same bits at 1, 2, 4 and 8 waves a workgroup, each in a process of its own;
  4. the object's call where its launch takes the LDS its largest K_i needs and not one byte more.

That every forgotten reset would show here is tests/test_pf_host.py's (the chain variants)."""
import hashlib
import math
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import pf_oracle as pf
from libstb_amd import capi
from test_gpu_pf import SENT_E, SENT_H, SENT_N, SENT_RES, SENT_T, SENT_W, assert_bits, assert_H, run_pf
from test_gpu_predict import dev, same_bits
from test_gpu_tdish import assert_state, fetch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("pn", "pt", "w", "E", "res", "Hi")


def run_full(R, tau):
    """stb_seat_filter on the whole launch into outputs filled with sentinels.  The outputs stay on the device (w alone is
    I x R doubles); returned are run_pf's dict restricted to the listed restaurants, in the compact case's layout, plus
    fillers: per output whether every restaurant that is not listed holds the closed form, and ms, the call's time"""
    import torch

    case, full = pf.chain_case()
    K, n, t, h, bpar, coff, cls, lik = case
    I, G = full["I"], int(full["koff"][-1]) * R
    listed = dev(full["listed"], np.int64)
    d_n, d_t = dev(n, np.uint32), dev(t, np.uint16)
    info = torch.zeros(5, dtype=torch.int64, device="cuda")
    out = {"Hi": torch.full((I,), SENT_H, dtype=torch.float64, device="cuda"),
           "w": torch.full((I, R), SENT_W, dtype=torch.float64, device="cuda"),
           "E": torch.full((I,), SENT_E, dtype=torch.int64, device="cuda"),
           "res": torch.full((I,), SENT_RES, dtype=torch.int32, device="cuda"),
           "pn": torch.full((G,), SENT_N, dtype=torch.int32, device="cuda"),
           "pt": torch.full((G,), SENT_T, dtype=torch.int16, device="cuda")}
    args = (pf.CHAIN_A, dev(full["bpar"], np.float64), dev(full["koff"], np.uint64), d_n, d_t, dev(full["coff"], np.uint64),
            dev(h, np.float64), 0, dev(cls, np.uint32), dev(lik, np.float64), R, tau, pf.SEED, pf.SWEEP)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    capi.seat_filter(*args, info=info, out=out)
    t1.record()
    torch.cuda.synchronize()
    rest = torch.ones(I, dtype=torch.bool, device="cuda")
    rest[listed] = False
    assert int(rest.sum()) == I - len(K)
    fillers = {"Hi": bool((out["Hi"][rest] == 0.0).all()), "w": bool((out["w"] == 1.0).all(dim=1)[rest].all()),
               "E": bool((out["E"][rest] == 0).all()), "res": bool((out["res"][rest] == 0).all())}
    got = {f: (out[f] if f in ("pn", "pt") else out[f][listed]).cpu().numpy() for f in FIELDS}
    got["res"], got["pn"], got["pt"] = got["res"].view(np.uint32), got["pn"].view(np.uint32), got["pt"].view(np.uint16)
    got.update({"info": tuple(int(v) for v in info.cpu().numpy()), "n": d_n.cpu().numpy().view(np.uint32),
                "t": d_t.cpu().numpy().view(np.uint16), "fillers": fillers, "ms": t0.elapsed_time(t1)})
    return got


def digest(gots):
    """the listed restaurants' outputs, the fillers' booleans and the counters of the three runs' full launches"""
    hsh = hashlib.sha256()
    for got in gots:
        for f in FIELDS:
            hsh.update(np.ascontiguousarray(got[f]).tobytes())
        hsh.update(repr((sorted(got["fillers"].items()), got["info"])).encode())
    return hsh.hexdigest()


@lru_cache(maxsize=None)
def launches(R, tau):
    """one full and one compact launch, the replay and the truth of the listed restaurants"""
    case, full = pf.chain_case()
    rep, Ht, Hb = pf.chain_truth(R, tau)
    got = run_full(R, tau)
    alone = run_pf(case, pf.CHAIN_A, 0, R, tau)
    print("R=%d tau=%g: %d restaurants on %d workgroups, %d listed; the call %.1f ms (its first in this process)"
          % (R, tau, full["I"], pf.GRID_CAP, len(case[0]), got["ms"]))
    return {"R": R, "tau": tau, "case": case, "rep": rep, "Ht": Ht, "Hb": Hb, "got": got, "alone": alone, "label": "chains R=%d tau=%g" % (R, tau)}


@pytest.fixture(scope="module", params=pf.CHAIN_RUNS, ids=lambda p: "R%d-tau%g" % p)
def chain(request):
    return launches(*request.param)


# ---- 1. the listed restaurants

def test_a_workgroups_second_and_third_restaurant_equal_the_replay(chain):
    got, rep = chain["got"], chain["rep"]
    assert capi.seat_filter_budget(130) == pf.budget(130) == 39 and capi.seat_filter_budget(128) == pf.budget(128) >= 40
    assert_bits(got, rep, chain["case"], chain["R"], chain["label"])     # skipped ones: sentinels; the counters; n and t
    assert rep["resamplings"] > 0 and rep["dead"] == 1 and got["info"][4] == rep["resamplings"]


def test_they_equal_a_launch_in_which_each_has_a_workgroup_of_its_own(chain):
    got, alone = chain["got"], chain["alone"]
    assert_bits(alone, chain["rep"], chain["case"], chain["R"], chain["label"] + " alone")
    for f in ("pn", "pt", "E", "res"):
        assert np.array_equal(got[f], alone[f]), (chain["label"], f)
    assert same_bits(got["w"], alone["w"]) and same_bits(got["Hi"], alone["Hi"]), (chain["label"], got["Hi"], alone["Hi"])
    assert got["info"] == alone["info"]


def test_their_H_lies_within_the_bar_of_the_truth(chain):
    exact = pf.chain_exact(chain["case"])
    assert len(exact) >= 6 and not np.isnan(chain["Ht"][exact]).any()
    assert_H(chain["got"], chain["rep"], chain["Ht"], chain["Hb"], chain["label"])
    assert_H(chain["alone"], chain["rep"], chain["Ht"], chain["Hb"], chain["label"] + " alone")


def test_the_fillers_hold_the_closed_form_and_are_not_counted(chain):
    got, rep = chain["got"], chain["rep"]
    assert got["fillers"] == {"Hi": True, "w": True, "E": True, "res": True}, (chain["label"], got["fillers"])
    assert got["info"][0] == rep["skipped"] == (5 if chain["R"] == 40 else 0)
    assert got["info"][3] == 1 and got["info"][4] == int(rep["res"].sum())


def test_a_skipped_restaurant_between_two_trips_keeps_its_sentinels(chain):
    got, rep, R = chain["got"], chain["rep"], chain["R"]
    K = chain["case"][0]
    koff = np.concatenate([[0], np.cumsum(K, dtype=np.int64)])
    assert list(np.flatnonzero(rep["skip"])) == ([i for i in range(len(K)) if K[i] == 130] if R == 40 else [])
    for i in np.flatnonzero(rep["skip"]):
        sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
        assert got["Hi"][i] == 0.0 and np.all(got["w"][i] == SENT_W) and got["E"][i] == SENT_E and got["res"][i] == SENT_RES, i
        assert np.all(got["pn"][sl] == SENT_N) and np.all(got["pt"][sl] == SENT_T), i


def test_a_dead_restaurant_does_not_kill_the_next(chain):
    got, alone, rep, m = chain["got"], chain["alone"], chain["rep"], pf.CHAIN_M
    d = pf.CHAIN_DEAD
    assert rep["dead_mask"][d] and got["Hi"][d] == -math.inf and not got["w"][d].any()
    for i in (d + m, d + 2 * m):
        assert math.isfinite(got["Hi"][i]) and got["Hi"][i] == alone["Hi"][i] and same_bits(got["w"][i], alone["w"][i]), i
        assert rep["skip"][i] or (got["w"][i] > 0.0).any(), i
    assert np.isfinite(np.delete(got["Hi"], d)).all()


def test_the_start_state_is_only_read(chain):
    n, t = chain["case"][1], chain["case"][2]
    for got in (chain["got"], chain["alone"]):
        assert np.array_equal(got["n"], n) and np.array_equal(got["t"], t)


# ---- 2. the waves

def test_three_trips_have_the_same_bits_whatever_the_waves_of_a_workgroup():
    # the three runs; of 39 slots seven of eight waves take five and one takes four.  A fresh process per setting, the
    # four at once
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--digest"],
                                 env=dict(env, STB_SEAT_WAVES=str(w)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for w in (1, 2, 4, 8)}
    out = {}
    for w, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (w, se[-2000:])
        out[w] = so.strip().splitlines()[-1]
    assert len(out[4]) == 64 and len(set(out.values())) == 1, out
    gots = [launches(R, tau)["got"] for R, tau in pf.CHAIN_RUNS]
    assert all(all(got["fillers"].values()) for got in gots) and out[4] == digest(gots)      # and this process, at the default


# ---- 3. the object at the budget's edge

def test_the_object_at_the_last_byte_of_its_budget_is_the_raw_call():
    a, tau = 0.45, 1.0
    shapes = [(130, 9), (3, 22), (65, 12), (64, 20)]
    K, n, t, h, bpar, coff, cls, lik = pf.make_case(shapes, a, 23)
    n0, t0 = np.maximum(n, 1).astype(np.uint32), np.maximum(t, 1).astype(np.uint16)     # (an object's pairs hold customers)
    t0 = np.minimum(t0, n0).astype(np.uint16)
    case = (K, n0, t0, h, bpar, coff, cls, lik)
    # the object's launch takes 12 R K' bytes for its largest K_i: at 39 particles all but 600 of the 61440, at 40 too many
    assert 12 * 39 * 130 == 60840 <= pf.LDS_DYN < 12 * 40 * 130 and pf.budget(130) == 39 and max(K) == 130
    ti = capi.TableIndicators(K, n0, t0, h)
    try:
        ti.set_lik(lik)
        ti.set_heldout(coff, cls)
        before = fetch(ti)
        for R, skipped in ((39, 0), (40, 1)):
            raw = run_pf(case, a, 0, R, tau, seed=31, sweep=2)
            tot_r, _, _ = capi.seat_loglik(raw["d_Hi"].reshape(-1, 1))
            tot, Hi, info = ti.heldout_pf(a, bpar, R, tau, 31, 2)
            assert same_bits(Hi, raw["Hi"]) and same_bits(tot, tot_r) and math.isfinite(tot), (R, Hi, raw["Hi"])
            assert (info.skipped, info.impossible, info.stuck, info.dead, info.resamplings) == raw["info"], R
            assert info.skipped == skipped and info.resamplings > 0 and info.customers == int(coff[-1])
            assert (Hi[0] == 0.0) == bool(skipped) and np.all(Hi[1:] < 0.0)
            assert_state(fetch(ti), before)
    finally:
        ti.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--digest"]:
        print(digest([run_full(R, tau) for R, tau in pf.CHAIN_RUNS]))
