"""CPU: the diversity statistics on the host (sat_amd/metrics.py: diversity_stats, diversity_per_hypothesis, diversity_from_stats -- the
specification of csrc/caption_diversity.hip) against worked values, distinct_n and corpus BLEU; the case generator; the two new C
entries' exports and argument checks (every check comes before a launch: no GPU is touched); CaptionStats carrying DiversityStats."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")

import diversity_cases as DC  # noqa: E402

WORKED = [([[1, 1, 1, 1], [1]], [1, 1, 1, 1, 5, 3, 2, 1, 2, 2, 2, 0, 0, 0, 5, 4, 3, 2, 5, 5]),
          ([[1, 2], [1, 2], [1, 2]], [2, 1, 0, 0, 6, 3, 0, 0, 3, 1, 6, 3, 0, 0, 6, 3, 3, 3, 6, 6]),
          ([[], []], [0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 0, 0, 0, 0, 2, 2, 2, 2, 0, 0]),
          ([[5, 6, 7]], [3, 2, 1, 0, 3, 2, 1, 0, 1, 1] + [0] * 10)]


def _m():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def _images():
    """every image of every shape, as the specification sees it"""
    return [image for K, W in DC.SHAPES for image in DC.clamped(DC.beams(K, W))]


def test_worked_rows():
    m = _m()
    for hyps, want in WORKED:
        assert m.diversity_stats(hyps) == want, hyps
    assert m.diversity_stats([]) == [0] * 20
    assert m.diversity_per_hypothesis([[1, 1, 1, 1], [1]]) == [[1, 0, 0, 0, 4, 3, 2, 1, 4, 1], [1, 0, 0, 0, 1, 1, 1, 1, 1, 4]]
    assert m.diversity_per_hypothesis([[5, 6, 7]]) == [[0] * 10] and m.diversity_per_hypothesis([]) == []
    assert m.DIVERSITY_STATS == 20 and len(WORKED[0][1]) == 20


def test_ratios_are_distinct_n():
    m = _m()
    for image in _images():
        s = m.diversity_stats(image)
        d = m.diversity_from_stats(s)
        for n in range(1, 5):
            assert (s[n - 1] / s[3 + n] if s[3 + n] else 0.0) == m.distinct_n(image, n) == d["distinct%d" % n], (image, n)
        assert s[8] == len(image) and s[9] == len(set(map(tuple, image)))
        assert d["hypotheses"] == len(image) and d["unique"] == (s[9] / s[8] if s[8] else 0.0) and "vocabulary" not in d


@pytest.mark.parametrize("K,W", DC.SHAPES)
def test_summed_columns_give_corpus_bleu_of_each_against_the_others(K, W):
    """bleu_from_stats of the columns summed over a shape's images == corpus_bleu over the (others, h_i) pairs, bit for bit"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    m = _m()
    assert m.MBLEU_WEIGHTS == {"m" + k: w for k, w in E.BLEU_WEIGHTS.items()}
    stats, per_hyp = DC.expected(K, W)
    sums = [sum(r[c] for r in stats) for c in range(20)]
    refs, hyps = [], []
    for image, rows, st in zip(DC.clamped(DC.beams(K, W)), per_hyp, stats):
        assert [sum(r[c] for r in rows) for c in range(10)] == st[10:], image
        if len(image) >= 2:
            for i, h in enumerate(image):
                refs.append(image[:i] + image[i + 1:]); hyps.append(h)
    d = m.diversity_from_stats(sums)
    for key, w in m.MBLEU_WEIGHTS.items():
        want = m.corpus_bleu(refs, hyps, w) if hyps else 0
        assert d[key] == want == m.bleu_from_stats(sums[10:14], sums[14:18], sums[18], sums[19], w), (K, W, key)
    if K >= 2 and W >= 4:
        assert 0.0 < d["mbleu1"] <= 1.0


def test_the_order_of_the_hypotheses_does_not_matter():
    m = _m()
    for hyps, want in WORKED:
        for perm in itertools.permutations(hyps):
            assert m.diversity_stats(list(perm)) == want
    for K, W in DC.SHAPES[:5]:
        for image, want in zip(DC.clamped(DC.beams(K, W)), DC.expected(K, W)[0]):
            assert m.diversity_stats(image[::-1]) == want and m.diversity_stats(image[1:] + image[:1]) == want, image


def test_from_stats_on_nothing():
    m = _m()
    d = m.diversity_from_stats([0] * 20, vocab_used=0)
    assert set(d) == set(m.DIVERSITY_KEYS) | {"vocabulary"} and all(v == 0 for v in d.values())
    assert set(m.diversity_from_stats([0] * 20)) == set(m.DIVERSITY_KEYS)
    one = m.diversity_from_stats(WORKED[3][1], vocab_used=3)             # one hypothesis: distinct-n and unique defined, mBLEU 0
    assert one["distinct1"] == 1.0 and one["distinct4"] == 0.0 and one["unique"] == 1.0 and one["mbleu1"] == 0 and one["mbleu4"] == 0
    assert one["vocabulary"] == 3
    with pytest.raises(ValueError):
        m.diversity_from_stats([0] * 12)


def test_the_generator_has_the_cases_it_claims():
    assert [s for s in DC.SHAPES] == [(1, 4), (2, 1), (3, 5), (5, 10), (7, 33), (32, 128)]
    for K, W in DC.SHAPES:
        hyps, has = DC.beams(K, W), DC.planted(K, W)
        tok, ln, cnt = DC.pack(hyps, K, W)
        assert len(hyps) <= DC.MAX_IMAGES and tok.shape == (len(hyps), K, W)
        assert all(len(h) <= K and all(len(c) <= W for c in h) for h in hyps)
        assert [len(h) for h in hyps[:K + 1]] == list(range(K + 1))                               # every count
        words = {t for h in hyps[:K + 6] + hyps[K + 7:] for c in h for t in c}
        assert words <= set(range(5)) and len(words) >= min(3, 1 + max(len(c) for h in hyps for c in h))
        if has["identical"]:
            assert len(hyps[K + 1]) >= 2 and len(set(map(tuple, hyps[K + 1]))) == 1 and len(hyps[K + 1][0]) >= 1
        assert len(hyps[K + 2]) >= 1 and all(c == [] for c in hyps[K + 2])                        # all empty
        lengths = {len(c) for h in hyps for c in h}
        assert set(range(min(4, W + 1))) <= lengths and W in lengths                              # shorter than n for every n; full width
        if has["clipping"]:
            assert hyps[K + 3][:2] == [[1, 1, 1, 1], [1]]
        if has["tie"]:
            a, lo, hi = (len(c) for c in hyps[K + 4][:3])
            assert a - lo == hi - a > 0 and all(len(c) in (a, lo, hi) for c in hyps[K + 4])
            assert DC.expected(K, W)[1][K + 4][0][9] == lo                                        # the tie went to the shorter
        assert cnt[K + 5] > K and ln[K + 5, 0] > W and cnt[0] < 0 and ln[K + 2, 0] < 0            # clamped on the device
        big = {t for c in hyps[K + 6] for t in c}
        assert ({65534, 65535, 70000} if W >= 3 or K >= 3 else {65534, 65535}) <= big               # (2, 1) has room for two tokens
        if W >= 4:
            assert -5 in big
        assert DC.clamped(hyps)[K + 6][0] == [65534, 65534, 65534, 0][:W]
        # the unused slots must not be read: they hold a word of the vocabulary and a full length
        assert (tok[1, 1:] == DC.GARBAGE).all() if K > 1 else True
        assert (ln[0] == W).all()
    # over the shapes together the statistics are not trivial: every column is non-zero somewhere, clipping bites, duplicates exist
    cols = [sum(r[c] for K, W in DC.SHAPES for r in DC.expected(K, W)[0]) for c in range(20)]
    assert all(c > 0 for c in cols) and cols[10] < cols[14] and cols[9] < cols[8] and cols[0] < cols[4]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_exports_declarations_and_bindings(lib):
    from sat_amd import _lib
    raw = ctypes.CDLL(os.path.join(PKG, "libsat_hip.so"))
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("sat_caption_diversity", "sat_caption_vocab_usage"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS and re.search(r"\bint %s\s*\(" % name, code), name
    assert "#define SAT_DIVERSITY_STATS 20" in header and _lib.DIVERSITY_STATS == 20
    lib.sat_abi_version.restype = ctypes.c_int
    assert lib.sat_abi_version() == 23 and "#define SAT_HIP_ABI_VERSION 23" in header          # symbols were added, nothing existing changed


def test_argument_checks_come_before_any_launch(lib):
    """null pointers and sizes beyond the limits return SAT_EINVAL (1) with text; B == 0 returns SAT_OK: no GPU is touched"""
    from sat_amd import _lib
    p = 4096                                                            # a non-null address: never dereferenced on the host
    err = lambda: lib.sat_last_error()
    dv = lambda **kw: lib.sat_caption_diversity(kw.get("tok", p), kw.get("len", p), kw.get("cnt", p), kw.get("B", 2), kw.get("K", 5), kw.get("W", 10),
                                                kw.get("stats", p), kw.get("per", p), None)
    for null in ("tok", "len", "cnt", "stats"):
        assert dv(**{null: None}) == 1 and b"caption_diversity: null" in err(), null
    assert dv(B=-1) == 1 and b"bad size" in err()
    assert dv(K=0) == 1 and b"bad size" in err()
    assert dv(W=0) == 1 and b"bad size" in err()
    assert dv(K=_lib.MBR_MAX_HYPS + 1) == 1 and b"over the limits" in err()
    assert dv(W=_lib.CAPTION_MAX_LEN + 1) == 1 and b"over the limits" in err()
    assert dv(B=0) == 0 and dv(B=0, per=None) == 0                       # nothing to do: no launch
    vu = lambda **kw: lib.sat_caption_vocab_usage(kw.get("tok", p), kw.get("len", p), kw.get("W", 10), kw.get("B", 2), kw.get("V", 60), kw.get("counts", p),
                                                  None)
    for null in ("tok", "len", "counts"):
        assert vu(**{null: None}) == 1 and b"caption_vocab_usage: null" in err(), null
    assert vu(V=0) == 1 and b"bad size" in err()
    assert vu(B=-1) == 1 and b"bad size" in err()
    assert vu(W=0) == 1 and b"cap_width" in err()
    assert vu(W=_lib.CAPTION_MAX_LEN + 1) == 1 and b"cap_width" in err()
    assert vu(B=0) == 0


def test_caption_stats_add_with_and_without_diversity():
    import torch
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    m = _m()

    def stats(div):
        return E.CaptionStats(torch.arange(12, dtype=torch.int64), torch.tensor(1.5, dtype=torch.float64), torch.tensor(6.0, dtype=torch.float64), 2,
                              diversity=div)

    def div(hyps, used, V=6):
        counts = torch.zeros(V, dtype=torch.int64)
        counts[used] = 2
        return E.DiversityStats(torch.tensor(m.diversity_stats(hyps), dtype=torch.int64), counts, 1, V)

    a, b = div(WORKED[0][0], [1]), div(WORKED[1][0], [1, 2])
    both = stats(a) + stats(b)
    assert both.images == 4 and both.diversity.images == 2 and both.diversity.vocab_size == 6
    assert both.diversity.sums.tolist() == [x + y for x, y in zip(WORKED[0][1], WORKED[1][1])]
    assert both.diversity.vocab_counts.tolist() == [0, 4, 2, 0, 0, 0]
    assert both.diversity.metrics() == m.diversity_from_stats(both.diversity.sums.tolist(), vocab_used=2)
    assert both.vector().shape == (14,) and E.metrics_from_vector(both.vector().tolist(), 4) == both.metrics()      # the layout is untouched
    assert (stats(None) + stats(None)).diversity is None
    for x, y in ((stats(a), stats(None)), (stats(None), stats(b))):
        with pytest.raises(ValueError, match="diversity"):
            x + y
    with pytest.raises(ValueError, match="vocabular"):
        a + div(WORKED[1][0], [1], V=7)
