"""AS 136 (k-means) and AS 241 (normal quantile): the C restatement (oracle/mpe_oracle.c) and the Python one
(oracle/clustermatepairs_oracle.py) against the answers of the REFERENCE'S OWN asa136.C / asa241.C, compiled as they lie
(oracle/Makefile: oracle/_ref/libasa_ref.so) and recorded on the inputs below by tests/golden/make_ref_answers.py into
tests/golden/ref_answers/asa.npz.  This is the one part of the clustermatepairs arithmetic that is pinned by the reference
itself."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers", "asa.npz")
# k <= 1 and m <= k: ifault 3
SMALL_KMNS = ((np.zeros(4), 2, 2, np.zeros(4), 2), (np.zeros(8), 4, 2, np.zeros(2), 1))


@pytest.fixture(scope="module")
def asa(built):
    from oracle import mpe_c
    return mpe_c


@pytest.fixture(scope="module")
def ref():
    """The reference's recorded answers; the inputs they were taken on must still be the ones generated here."""
    d = dict(np.load(GOLDEN))
    assert str(d["inputs_sha256"]) == inputs_digest(), "the test inputs changed since asa.npz was recorded: tests/golden/make_ref_answers.py"
    return d


def kmns_cases():
    rng = np.random.default_rng(136)
    for trial in range(400):
        m = int(rng.integers(3, 120))
        k = int(rng.integers(2, min(10, m - 1) + 1))
        kind = trial % 5
        if kind == 0:                                    # blobs
            cen = rng.normal(0, 500, size=(k, 2))
            pts = cen[rng.integers(0, k, size=m)] + rng.normal(0, 30, size=(m, 2))
        elif kind == 1:                                  # integer coordinates with duplicates (what the tool feeds)
            pts = rng.integers(-50, 50, size=(m, 2)).astype(np.float64) + np.array([37000.0, -29000.0])
        elif kind == 2:                                  # a line: many equal distances
            pts = np.stack([np.arange(m) * 10.0, np.zeros(m)], axis=1)
        elif kind == 3:                                  # two far groups, k larger than the groups
            pts = np.concatenate([rng.normal(0, 5, size=(m // 2, 2)), rng.normal(10000, 5, size=(m - m // 2, 2))])
        else:
            pts = rng.random(size=(m, 2))
        seeds = pts[rng.choice(m, size=k, replace=False)] if trial % 7 else pts[:k]
        yield m, k, pts, seeds


def cdf_points():
    rng = np.random.default_rng(241)
    return np.array(list(rng.random(20000)) + [0.025, 0.005, 0.0005, 1e-10, 1e-300, 1 - 1e-12, 0.075, 0.925, 0.5, 0.0, 1.0, -1.0, 2.0,
                                                (1 - 0.95) / 2, (1 - 0.99) / 2, (1 - 0.9) / 2], dtype=np.float64)


def inputs_digest():
    h = hashlib.sha256()
    for m, k, pts, seeds in kmns_cases():
        h.update(np.array([m, k], dtype=np.int64).tobytes() + pts.astype(np.float64).tobytes() + seeds.astype(np.float64).tobytes())
    h.update(cdf_points().tobytes())
    return h.hexdigest()


def ref_kmns_answers(ref):
    """The reference's (ic1, nc, wss, c, ifault) per case of kmns_cases(), in order."""
    o = dict.fromkeys(("ic1", "nc", "wss", "c"), 0)
    for i, (m, k) in enumerate(zip(ref["m"], ref["k"])):
        m, k = int(m), int(k)
        sizes = {"ic1": m, "nc": k, "wss": k, "c": 2 * k}
        got = {}
        for key, n in sizes.items():
            got[key] = ref[key][o[key]:o[key] + n]
            o[key] += n
        yield got["ic1"], got["nc"], got["wss"], got["c"], int(ref["fault"][i])


def test_kmns_restatements_equal_the_reference(asa, ref):
    from oracle import clustermatepairs_oracle as o
    n_checked = n_fault1 = 0
    cases = list(kmns_cases())
    answers = list(ref_kmns_answers(ref))
    assert len(answers) == len(cases)
    for (m, k, pts, seeds), (r_ic1, r_nc, r_wss, r_c, r_fault) in zip(cases, answers):
        a = np.concatenate([pts[:, 0], pts[:, 1]])       # column-major a[i + j*m]
        c = np.concatenate([seeds[:, 0], seeds[:, 1]])
        o_ic1, o_nc, o_wss, o_c, o_fault = asa.kmns(a, m, 2, c, k)
        assert o_fault == r_fault
        if r_fault == 1:                                 # a seed attracted no point: outputs are not defined beyond ic1 / nc
            n_fault1 += 1
            assert (o_ic1 == r_ic1).all() and (o_nc == r_nc).all()
            continue
        assert (o_ic1 == r_ic1).all() and (o_nc == r_nc).all()
        assert o_c.tobytes() == r_c.tobytes() and o_wss.tobytes() == r_wss.tobytes()      # bit for bit
        if m <= 40:                                      # the Python restatement is slow
            cc = list(c)
            p_ic1, p_nc, p_wss, p_fault = o.kmns(list(a), m, 2, cc, k, 1000)
            assert p_fault == r_fault and p_ic1 == list(r_ic1) and p_nc == list(r_nc)
            assert np.array(cc).tobytes() == r_c.tobytes() and np.array(p_wss).tobytes() == r_wss.tobytes()
        n_checked += 1
    assert n_checked > 300
    assert [int(f) for f in ref["fault_small"]] == [3, 3]
    for args in SMALL_KMNS:
        assert asa.kmns(*args)[4] == 3


def test_cdf_inverse_equals_the_reference(asa, ref):
    from oracle import clustermatepairs_oracle as o
    ps = cdf_points()
    assert ps.tobytes() == ref["cdf_p"].tobytes()
    for p, r in zip(ps.tolist(), ref["cdf_inverse"].tolist()):
        assert asa.lib().ora_cdf_inverse(p) == r
        assert o.normal_01_cdf_inverse(p) == r


def test_cdf_inverse_on_the_reference_table(asa, ref):
    """asa241.C carries its own known-answer table (normal_01_cdf_values, :13-113): x and CDF(x) to 16 digits.  The inverse
    must bring every tabulated CDF value back to its x."""
    seen = 0
    for x, fx in zip(ref["table_x"].tolist(), ref["table_fx"].tolist()):
        seen += 1
        assert abs(asa.lib().ora_cdf_inverse(fx) - x) < 1e-13 * max(1.0, abs(x)) + 2e-14 / max(1e-3, fx * (1 - fx))
    assert seen >= 10


def test_min_probability_of_the_tool():
    """mMinProbability (tools/MatePairEM.cpp:49-50) as the tool computes it on the host, against both restatements."""
    from oracle import clustermatepairs_oracle as o, mpe_c
    for sd, prec in ((30.0, 0.95), (45.0, 0.95), (30.0, 0.99), (12.5, 0.5)):
        assert mpe_c.lib().ora_min_probability(sd, prec) == o.MatePairEM(300.0, sd, prec, 5).min_prob
