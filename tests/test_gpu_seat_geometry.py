"""k_seat_sum and k_seat (libstb_amd/csrc/seat.hip) past one block, one chunk of particles, one staging trip and one
grid-stride step; a dish at the uint16 bound; the object's held-out seating at more than one block.

  1. stb_seat_loglik on synthetic log weights (st_oracle.lw_types, exact doubles): every H_i within the derived bar
     (st_oracle.loglik_rows_bar) of the long-double truth, and the total bit for bit st_oracle.loglik_total of the
     device's own H_i -- the kernel's association leaves no rounding freedom once the H_i are given.  The sizes come from
     stb_reduce_geometry and every test asserts what the query says before it relies on it.
  2. stb_seat_customers with 2^20 + 64 items: at one wave a workgroup the last restaurant's particles are the grid-stride
     loop's second step.
  3. four restaurants whose pinned dish starts at t = 65534 and 65535 under M = 0.
  4. stb_tindic_heldout_seq on 300 restaurants and 65 particles against the raw calls.

The oracle's own checks, the wrong variants included, are tests/test_seat_host.py's."""
import math

import numpy as np
import pytest

import st_oracle as sto
from libstb_amd import capi
from test_gpu_predict import dev, same_bits
from test_gpu_seat import loglik, run_raw
from test_gpu_tdish import random_lik, random_state

pytestmark = pytest.mark.gpu


def geom(I, waves=0):
    return capi.reduce_geometry(capi.GEOM_LOGJOINT, I, waves=waves)


def show(what, g, **kw):
    print(what, "blocks", g.blocks, "grid_x", g.grid_x, "steps", g.steps, "waves", g.waves, "need", g.need, "cap0", g.cap0,
          " ".join(f"{k} {v}" for k, v in kw.items()))


def big_I():
    return sto.past_one_block(int(geom(1 << 30).grid_x))


def tiled(types, I):
    """restaurant i of row type i mod 257, made on the device"""
    import torch

    d = dev(types, np.float64)
    return d[torch.arange(I, device="cuda") % types.shape[0]].contiguous()


@pytest.fixture(scope="module")
def types3():
    """(the 257 types at R = 3, their truth, the bars, the device's H_i of the 257 alone -- held to the truth here)"""
    lw = sto.lw_types(3)
    tr = sto.loglik_rows_truth(lw)
    bar = sto.loglik_rows_bar(lw, tr)
    tot, Hi, info = loglik(dev(lw, np.float64))
    ratio = sto.over_bar(Hi, tr, bar)
    print("the 257 types alone, R = 3: largest H_i error over bar", ratio)
    assert ratio <= 1.0 and info.impossible == 0 and same_bits(tot, sto.loglik_total(Hi))
    return lw, tr, bar, Hi


def check_call(d_lw, tr_types, bar_types, what, g):
    """one stb_seat_loglik on rows tiled from the types: every H_i within the bar of the truth (a dead row -inf exactly),
    the counter, the total bit for bit from the device's H_i and within the total bar of the truth's sum.  Returns
    (total, H_i)"""
    I = int(d_lw.shape[0])
    tot, Hi, info = loglik(d_lw)
    tr, bar = np.resize(tr_types, I), np.resize(bar_types, I)
    ndead = int((tr == -math.inf).sum())
    ratio = sto.over_bar(Hi, tr, bar)
    ttot, tbar = sto.loglik_total_truth(tr, bar)
    show(what, g, I=I, R=int(d_lw.shape[1]), dead=ndead, H_i_error_over_bar=ratio, total=tot,
         total_error_over_bar=0.0 if ndead else abs(float(tot - ttot)) / tbar)
    assert ratio <= 1.0 and not np.isnan(Hi).any(), (what, ratio)
    assert np.array_equal(Hi == -math.inf, tr == -math.inf)
    assert (info.skipped, info.impossible, info.stuck, info.customers) == (0, ndead, 0, 0)
    assert same_bits(tot, sto.loglik_total(Hi)), (what, tot, sto.loglik_total(Hi))
    assert tot == -math.inf if ndead else abs(tot - ttot) <= tbar, (what, tot, ttot, tbar)
    return tot, Hi


# ---- 1. stb_seat_loglik on synthetic log weights

@pytest.mark.parametrize("R", (1, 2, 63, 64, 65, 127, 128, 129, 4096))
def test_particle_counts_past_one_base_of_64(R):
    I = 257 + 256
    g = geom(I)
    assert g.blocks == 3 and g.need == 3 <= g.cap0 and I % 256 == 1        # three blocks, the last of one restaurant
    for dead_row in (False, True):
        lw = sto.lw_types(R, dead_row=dead_row)
        tr = sto.loglik_rows_truth(lw)
        tot, Hi = check_call(tiled(lw, I), tr, sto.loglik_rows_bar(lw, tr), f"particles, dead row {dead_row}:", g)
        assert same_bits(Hi, np.resize(Hi[:257], I))                       # a row's H_i does not depend on where it sits
        assert (tot == -math.inf) == dead_row


def test_a_workgroup_takes_a_second_block(types3):
    import torch

    lw, tr, bar, H_types = types3
    I = big_I()
    g = geom(I)
    assert g.steps > g.grid_x and g.blocks == g.steps and g.need <= g.cap0 and I >= 70000
    d_lw = tiled(lw, I)
    tot, Hi = check_call(d_lw, tr, bar, "past one block a workgroup:", g)
    assert same_bits(Hi, np.resize(H_types, I))
    # dead rows: in the first block, in a middle one, in the first block a workgroup takes on its second step, in the last
    dead = sorted({7, (g.grid_x // 2) * 256 + 100, g.grid_x * 256, I - 1})
    # (where the grid is one block short of the blocks the last two are one row, the last block's one restaurant)
    assert g.grid_x * 256 < I and dead[-1] // 256 == g.blocks - 1 >= g.grid_x and dead[1] // 256 not in (0, g.blocks - 1)
    d_lw[torch.as_tensor(dead, device="cuda")] = -math.inf
    tot_d, Hi_d, info = loglik(d_lw)
    show("the same with dead rows:", g, rows=dead, counted=info.impossible, total=tot_d)
    assert tot_d == -math.inf and info.impossible == len(dead)
    want = np.resize(H_types, I)
    want[dead] = -math.inf
    assert same_bits(Hi_d, want)


def test_a_second_base_and_a_second_block_at_once():
    I, R = big_I(), 65
    g = geom(I)
    assert g.steps > g.grid_x
    lw = sto.lw_types(R)
    tr = sto.loglik_rows_truth(lw)
    bar = sto.loglik_rows_bar(lw, tr)
    _, H_types = check_call(dev(lw, np.float64), tr, bar, "the 257 types alone, R = 65:", geom(257))
    tot, Hi = check_call(tiled(lw, I), tr, bar, "past one base and one block:", g)
    assert same_bits(Hi, np.resize(H_types, I))


def test_the_sum_has_the_same_bits_for_every_workgroup_size(types3, monkeypatch):
    lw, tr, bar, H_types = types3
    I = big_I()
    d_lw = tiled(lw, I)
    seen = {}
    for w in (1, 2, 4, 8):
        monkeypatch.setenv("STB_SEAT_WAVES", str(w))                       # (read at every call)
        g = geom(I, w)
        assert g.waves == w and g.steps > g.grid_x
        tot, Hi = check_call(d_lw, tr, bar, f"STB_SEAT_WAVES={w}:", g)
        seen[w] = (np.float64(tot).tobytes(), Hi.tobytes())
    assert len(set(seen.values())) == 1 and same_bits(np.frombuffer(seen[1][1]), np.resize(H_types, I))


def test_the_block_sums_outgrow_their_first_buffer_and_the_calls_after_it():
    cap0 = int(geom(1).cap0)
    big, small = cap0 * 256 + 1, 257
    gb, gs = geom(big), geom(small)
    assert gb.need == gb.cap0 + 1 == gb.blocks and gb.blocks > 2 * sto.STAGE and gs.need == 2 <= gs.cap0
    lw = sto.lw_types(1)
    tr = sto.loglik_rows_truth(lw)
    bar = sto.loglik_rows_bar(lw, tr)
    d_big, d_small = tiled(lw, big), dev(lw, np.float64)

    def run(d, what, g):
        tot, Hi = check_call(d, tr, bar, what, g)
        assert same_bits(Hi, np.resize(lw[:, 0], len(Hi)))                 # one particle: H_i = lw_i + log(1)
        return np.float64(tot).tobytes(), Hi.tobytes()

    capi.lib().stb_sampler_cache_clear()     # (this thread's buffer of block sums: the next call allocates afresh)
    try:
        ref_b = run(d_big, "regrow:", gb)                                  # more than the first buffer would hold
        ref_s = run(d_small, "after the larger call:", gs)                 # a smaller call in the larger buffer
        assert run(d_big, "the large call again:", gb) == ref_b
        capi.lib().stb_sampler_cache_clear()
        assert run(d_small, "the small call in a first buffer:", gs) == ref_s
    finally:
        capi.lib().stb_sampler_cache_clear()


# ---- 2. k_seat past its grid cap

def run_grid(particles=sto.GRID_R):
    return run_raw(sto.grid_case(), sto.GRID_A, 0, particles, seed=sto.GRID_SEED, sweep=sto.GRID_SWEEP)


@pytest.fixture(scope="module")
def grid_one_wave():
    """the grid case at one wave a workgroup: the launch whose last 64 items are a second grid-stride step"""
    items = sto.GRID_I * sto.GRID_R
    assert items > sto.GRID_CAP and items - sto.GRID_CAP == sto.GRID_R
    mp = pytest.MonkeyPatch()
    mp.setenv("STB_SEAT_WAVES", "1")
    try:
        got = run_grid()
    finally:
        mp.undo()
    print("k_seat at one wave a workgroup:", items, "items on", sto.GRID_CAP, "workgroups, a second step of", items - sto.GRID_CAP)
    assert got["lw"].shape == (sto.GRID_I, sto.GRID_R) and np.isfinite(got["lw"]).all() and got["info"] == (0, 0, 0)
    return got


def test_the_second_grid_stride_step_has_the_bits_of_a_launch_without_one(grid_one_wave, monkeypatch):
    items = sto.GRID_I * sto.GRID_R
    for w in (2, 4, 8):
        assert -(-items // w) < sto.GRID_CAP                               # one step
        monkeypatch.setenv("STB_SEAT_WAVES", str(w))
        got = run_grid()
        assert same_bits(got["lw"], grid_one_wave["lw"]) and got["info"] == grid_one_wave["info"], w
    monkeypatch.setenv("STB_SEAT_WAVES", "1")
    one = run_grid(1)
    assert same_bits(one["lw"][:, 0], grid_one_wave["lw"][:, 0])            # particle 0 is the call of one particle


def test_the_band_around_the_second_step_lies_within_the_bars(grid_one_wave):
    band, rep, tr = sto.grid_band_truth()
    assert band[-1] == sto.GRID_I - 1 == sto.GRID_CAP // sto.GRID_R and rep["impossible"] == 0
    lw = grid_one_wave["lw"]
    worst = 0.0
    for i in band:
        for r in range(sto.GRID_R):
            assert sto.within(lw[i, r], tr["lw"][i, r], tr["lw_bar"][i, r]), (i, r, lw[i, r], tr["lw"][i, r], tr["lw_bar"][i, r])
            worst = max(worst, abs(lw[i, r] - tr["lw"][i, r]) / tr["lw_bar"][i, r])
    print("band of", len(band), "restaurants x", sto.GRID_R, "particles: largest lw error over bar", worst)


def test_the_register_form_takes_the_second_step_too(grid_one_wave, monkeypatch):
    K, n, t, h, bpar, coff, cls, lik = sto.grid_case()
    monkeypatch.setenv("STB_SEAT_WAVES", "1")
    tot_r, Hi_r, _ = loglik(grid_one_wave["d_lw"])
    ti = capi.TableIndicators(K, n, t, h)        # its largest K is 2: k_seat<true>
    try:
        ti.set_lik(lik)
        ti.set_heldout(coff, cls)
        tot, Hi, info = ti.heldout_seq(sto.GRID_A, bpar, sto.GRID_R, sto.GRID_SEED, sto.GRID_SWEEP)
        assert same_bits(Hi, Hi_r) and same_bits(tot, tot_r) and math.isfinite(tot)
        assert (info.skipped, info.impossible, info.stuck, info.customers) == grid_one_wave["info"] + (int(coff[-1]),)
        n1, _ = ti.get_state()
        assert np.array_equal(n1, n)
    finally:
        ti.free()


# ---- 3. a dish at the uint16 bound

def test_a_dish_at_65534_opens_one_table_and_none_at_65535():
    case = sto.bound_case()
    K = case[0]
    rp = sto.bound_replay()
    opened = sto.bound_opened(rp)
    assert [o[0] for o in opened] == [1, 0, 1, 0] and all(o[2] == 65535 for o in opened) and opened[0][1] >= 2 <= opened[2][1]
    got = run_raw(case, sto.BOUND_A, 0, 1, commit=True, seed=sto.BOUND_SEED, sweep=sto.BOUND_SWEEP)
    for f in ("n", "t", "T", "cust"):
        assert np.array_equal(got[f], rp[f]), (f, got[f], rp[f])
    assert same_bits(got["p"], rp["p"]) and got["info"] == (0, 0, 0)
    koff = np.concatenate([[0], np.cumsum(K)])
    assert [int(got["t"][koff[i + 1] - 1]) for i in range(4)] == [65535] * 4
    assert [int(v) for v in got["T"]] == [o[3] for o in opened]
    assert np.isfinite(got["lw"]).all()
    # not committed: the same weights, nothing written
    free = run_raw(case, sto.BOUND_A, 0, 2, seed=sto.BOUND_SEED, sweep=sto.BOUND_SWEEP)
    assert same_bits(free["lw"][:, 0], got["lw"][:, 0]) and np.array_equal(free["t"], case[2]) and np.array_equal(free["n"], case[1])


# ---- 4. the object at more than one block

def test_an_empty_object_of_two_blocks_scores_unseen_documents_as_the_raw_call():
    a, R = 0.45, 65
    rng = np.random.default_rng(17)
    Ks = list(rng.integers(1, 10, size=297)) + [70, 64, 65]
    K, n, t, h = random_state(rng, Ks, 6)
    coff = np.concatenate([[0], np.cumsum([x.sum() for x in np.split(n.astype(np.int64), np.cumsum(K)[:-1])])]).astype(np.uint64)
    cls = rng.integers(0, 3, size=int(coff[-1])).astype(np.uint32)
    lik = random_lik(rng, 3, int(K.max()) + 3)
    bpar = 0.3 + 4.0 * rng.random(len(K))
    zn, zt = np.zeros_like(n), np.zeros_like(t)
    g = geom(len(K))
    assert len(K) == 300 and g.blocks == 2
    raw = run_raw((K, zn, zt, h, bpar, coff, cls, lik), a, 0, R, seed=31, sweep=2)
    tot_r, Hi_r, info_r = loglik(raw["d_lw"])
    show("the object against the raw calls:", g, R=R, total=tot_r, impossible_visits=raw["info"][1], dead_rows=info_r.impossible)
    assert same_bits(tot_r, sto.loglik_total(Hi_r)) and info_r.impossible == int((Hi_r == -math.inf).sum())
    # every theta is positive (h > 0, no truncation), so a visit is impossible exactly where its class's row is zero on
    # all the restaurant's dishes, whatever the path: the dead rows are known without a replay
    dead = np.array([any(not lik[w, :K[i]].any() for w in cls[int(coff[i]):int(coff[i + 1])]) for i in range(len(K))])
    assert np.array_equal(Hi_r == -math.inf, dead) and not np.isnan(Hi_r).any() and 0 < dead.sum() < 100
    ti = capi.TableIndicators(K, zn, zt, h)
    try:
        ti.set_lik(lik)
        ti.set_heldout(coff, cls)
        tot, Hi, info = ti.heldout_seq(a, bpar, R, 31, 2)
        assert same_bits(Hi, Hi_r) and same_bits(tot, tot_r)
        assert (info.skipped, info.impossible, info.stuck, info.customers) == (0,) + raw["info"][1:] + (int(coff[-1]),)
        n1, _ = ti.get_state()
        assert not n1.any()
    finally:
        ti.free()
