"""The Gaussian-observation steps' replay (tests/gs_oracle.py) against the mathematics, on the CPU: the evidence's closed
form against the chain rule of Student-t predictives and against Bayes' identity in 40 digits, the two-pass statistics
inside the bar of their own operations where the one-pass form is many bars out, and the law of the replayed draw."""
import math

import numpy as np
import pytest

import gs_oracle as gso
import hq_oracle as hqo
import tl_oracle as tlo

KS_BAR = 1.95   # sqrt(n) D of Kolmogorov's law at p = 1e-3


def mp():
    return gso._mp()


# ---- 1. the identity ----

def mp_log_student(x, nu, loc, lam):
    """log density of Student-t with nu degrees of freedom, location loc and precision lam"""
    m = mp()
    return (m.loggamma((nu + 1) / 2) - m.loggamma(nu / 2) + m.log(lam / (m.pi * nu)) / 2
            - (nu + 1) / 2 * m.log(1 + lam * (x - loc) ** 2 / nu))


def mp_posterior(xs, k0, a0, b0, m0):
    m = mp()
    n, mean, Q = gso.mp_stats(xs)
    kn = k0 + n
    return kn, (k0 * m0 + n * mean) / kn, a0 + m.mpf(n) / 2, b0 + Q / 2 + k0 * n * (mean - m0) ** 2 / (2 * kn)


def mp_log_normal_gamma(mu, tau, k, mloc, a, b):
    m = mp()
    return (a * m.log(b) - m.loggamma(a) + (a - 1) * m.log(tau) - b * tau
            + m.log(k * tau / (2 * m.pi)) / 2 - k * tau * (mu - mloc) ** 2 / 2)


def test_the_evidence_is_the_chain_rule_and_bayes_identity():
    m = mp()
    rng = np.random.default_rng(1)
    for n, (k0, a0, b0, m0) in ((1, (0.7, 0.4, 1.3, -0.5)), (5, (2.0, 2.5, 0.6, 1.0)), (12, (0.01, 7.0, 3.0, 0.0))):
        xs = [float(v) for v in rng.normal(0.3, 1.7, size=n)]
        k0, a0, b0, m0 = (m.mpf(v) for v in (k0, a0, b0, m0))
        nn, mean, Q = gso.mp_stats(xs)
        ev = gso.mp_logml_cell(nn, mean, Q, k0, a0, b0, m0)
        # the chain rule: x_{j+1} | x_1..j is Student-t(2 alpha_j, m_j, alpha_j kappa_j / (beta_j (kappa_j + 1)))
        chain = m.mpf(0)
        for j in range(n):
            kj, mj, aj, bj = mp_posterior(xs[:j], k0, a0, b0, m0)
            chain += mp_log_student(m.mpf(xs[j]), 2 * aj, mj, aj * kj / (bj * (kj + 1)))
        assert abs(ev - chain) < m.mpf(10) ** -30, (n, ev - chain)
        # Bayes: p(x) = p(x | mu, tau) p(mu, tau) / p(mu, tau | x) at any (mu, tau)
        kn, mn, an, bn = mp_posterior(xs, k0, a0, b0, m0)
        for mu, tau in ((m.mpf("0.37"), m.mpf("0.9")), (m.mpf(-3), m.mpf("12.5"))):
            like = m.fsum(m.log(tau / (2 * m.pi)) / 2 - tau * (m.mpf(v) - mu) ** 2 / 2 for v in xs)
            bayes = like + mp_log_normal_gamma(mu, tau, k0, m0, a0, b0) - mp_log_normal_gamma(mu, tau, kn, mn, an, bn)
            assert abs(ev - bayes) < m.mpf(10) ** -30, (n, ev - bayes)


def test_the_replayed_totals_lie_within_their_bars_of_the_truth():
    rng = np.random.default_rng(2)
    C, K, D = 300, 4, 3
    cust = rng.integers(0, K + 1, size=C)
    x = rng.normal(0.0, 2.0, size=(C, D)) + cust[:, None]
    pr = gso.prior(0.7, 0.4, [0.5, 1.0, 2.0], D, m0=[0.1, -0.2, 0.3])
    n, mean, Q, skipped = gso.stats(x, cust, K)
    mu, tau, _ = gso.draw(n, mean, Q, pr, 5, 0)
    tot, sk = gso.loglik(x, cust, mu, tau)
    err, bar = abs(float(mp().mpf(tot) - gso.mp_loglik(x, cust, mu, tau))), gso.loglik_bar(x, cust, mu, tau)
    print("data term", tot, "error", err, "bar", bar)
    assert sk == skipped == int((cust >= K).sum()) and err <= bar
    ml = gso.logml(n, mean, Q, pr)
    err, bar = abs(float(mp().mpf(ml) - gso.mp_logml(n, mean, Q, pr))), gso.logml_bar(n, mean, Q, pr)
    print("evidence", ml, "error", err, "bar", bar)
    assert err <= bar


# ---- 2. the statistics ----

def test_two_passes_stay_inside_their_bar_where_one_pass_is_many_bars_out():
    rng = np.random.default_rng(3)
    n = 300
    x = (1e8 + rng.normal(0.0, 1.0, size=n)).reshape(n, 1)
    cust = np.zeros(n, dtype=np.uint32)
    cnt, mean, Q, _ = gso.stats(x, cust, 1)
    _, tmean, tQ = gso.mp_stats(x[:, 0])
    bar = gso.Q_bar(x[:, 0], float(mean[0, 0]))
    err = abs(float(mp().mpf(float(Q[0, 0])) - tQ))
    wrong = abs(float(mp().mpf(float(gso.one_pass_Q(x, cust, 1)[0, 0])) - tQ))
    print("Q", float(Q[0, 0]), "two passes: error", err, "bar", bar, " one pass: error", wrong, "=", wrong / bar, "bars")
    assert cnt[0] == n and err <= bar
    assert wrong > 1e6 * bar
    assert abs(float(mp().mpf(float(mean[0, 0])) - tmean)) <= gso.U * 1e8 * (gso.CHUNK + 2)


def test_the_replays_association_is_the_headers():
    # 600 customers of one dish in three chunks: the chunk partials by hand
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, size=(600, 1)) * 10.0 ** rng.integers(-8, 8, size=(600, 1))
    cust = np.zeros(600, dtype=np.uint32)
    cust[256:512] = 7                                  # the middle chunk has no member: skipped
    cust[5] = 9
    parts = []
    for c0 in (0, 512):
        s = None
        for c in range(c0, min(c0 + 256, 600)):
            if cust[c] == 0:
                s = x[c, 0] if s is None else s + x[c, 0]
        parts.append(s)
    hi, lo = gso.dd_add(0.0, 0.0, parts[0])
    hi, lo = gso.dd_add(hi, lo, parts[1])
    S, n = gso.dish_sums(x, cust, 1)
    assert n[0] == 600 - 256 - 1 and S[0, 0] == hi + lo
    # the double-double keeps what a plain sum of the partials loses
    assert gso.dd_add(1e16, 0.0, 1.0) == (1e16, 1.0)
    # the counted log-Gamma replay is tl_oracle's
    keys = tlo.cell_keys(9, 1, 500)
    alpha = np.concatenate([np.full(250, 0.3), np.linspace(1.0, 40.0, 250)])
    a, _ = tlo.log_gamma(alpha, keys)
    b, k, _ = gso.log_gamma_counted(alpha, keys)
    assert np.array_equal(a, b) and k.min() >= 3 and (k[:250] >= 4).all()


# ---- 3. the law of the draw ----

def test_the_law_of_the_replayed_draw():
    m = mp()
    m.mp.dps = 20
    try:
        xs = np.array([-1.2, 0.4, 0.9, 2.5, 3.1]).reshape(5, 1)
        pr = gso.prior(0.8, 0.6, 1.4, 1, m0=[0.5])
        n, mean, Q, _ = gso.stats(xs, np.zeros(5, dtype=np.uint32), 1)
        kn, mn, an, bn = (float(v[0, 0]) for v in gso.posterior(n, mean, Q, pr))
        mus, taus, worst = np.empty(2000), np.empty(2000), math.inf
        for s in range(2000):
            mu, tau, margin = gso.draw(n, mean, Q, pr, 8100, s)
            mus[s], taus[s], worst = mu[0, 0], tau[0, 0], min(worst, margin)
        # tau ~ Gamma(alpha_n, rate beta_n); mu ~ Student-t(2 alpha_n, m_n, precision alpha_n kappa_n / beta_n)
        p_tau = [float(m.gammainc(an, 0, bn * t, regularized=True)) for t in taus]
        lam = an * kn / bn

        def t_cdf(v):
            z = (v - mn) * math.sqrt(lam)
            nu = 2.0 * an
            tail = 0.5 * float(m.betainc(nu / 2, 0.5, 0, nu / (nu + z * z), regularized=True))
            return 1.0 - tail if z > 0 else tail

        p_mu = [t_cdf(v) for v in mus]
        ks_tau, ks_mu = hqo.ks_stat(p_tau), hqo.ks_stat(p_mu)
        print("sqrt(n) D: tau", ks_tau, "mu", ks_mu, "smallest margin", worst)
        assert ks_tau <= KS_BAR and ks_mu <= KS_BAR and worst > 1e-9
        # they can fail: tau read as a variance, and kappa_n left out of mu's spread
        assert hqo.ks_stat([float(m.gammainc(an, 0, bn / t, regularized=True)) for t in taus]) > 5.0
        lam = an / bn
        assert hqo.ks_stat([t_cdf(v) for v in mus]) > 5.0
    finally:
        m.mp.dps = 40


# ---- 4. the law of the chain ----

def chain_pvalue(law, which):
    import ch_oracle as ch

    (k0, a0, b0), iterations = gso.CHAIN_PRIORS[which]
    pr = gso.prior(k0, a0, b0, 1)
    index, probs = ch.merge_cells(gso.chain_exact(pr), (iterations - gso.CHAIN["burn"]) // gso.CHAIN["thin"])
    kept, worst = gso.chain_run(law, pr, iterations)
    p = ch.chi2_pvalue(ch.cell_counts(kept, index, len(probs)), probs)
    print(law, which, "bins", len(probs), "kept", len(kept), "p", p, "smallest margin", worst)
    return p, worst


@pytest.mark.parametrize("which", list(gso.CHAIN_PRIORS))
def test_the_chain_has_the_enumerated_law(which):
    """dish sweep (td_oracle) under the replayed matrix, alternated with the redraw, against the exact p(z | x) of 2
    restaurants x 3 customers x 2 dishes: the PYP prior times the evidence, over the partitions of the six customers"""
    p, worst = chain_pvalue("right", which)
    assert p > 1e-3 and worst > 1e-9


@pytest.mark.parametrize("law", list(gso.CHAIN_WRONG))
def test_a_wrong_chain_is_told_apart(law):
    p, _ = chain_pvalue(law, gso.CHAIN_WRONG[law])
    assert p < 1e-6
