"""CPU: consensus (minimum-Bayes-risk) reranking on the host (sat_amd/metrics.py: consensus_utilities, the specification of
csrc/caption_mbr.hip) against the worked example and hand-computed edge cases, the three new C entries' exports and argument checks
(every check comes before a launch: no GPU is touched), the Python refusals, and random_search's draws against a recording."""
import ctypes
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")

import mbr_cases as MC  # noqa: E402
from consensus_cases import REFS  # noqa: E402

#: two images without a common n-gram: every n-gram of a reference has df 1 and weighs log 2 (tests/test_consensus.py)
TWO = [[[1, 2]], [[3, 4]]]


def _m():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def test_worked_example_bit_for_bit():
    m = _m()
    df = m.document_frequency(REFS)
    for reward, alpha, want, winner in MC.WORKED:
        got = m.consensus_utilities(MC.HYPS, MC.LOGPS, df, 4, reward=reward, alpha=alpha)
        assert got == want, (reward, alpha, got)
        assert got.index(max(got)) == winner
    # hypothesis 3 has the best raw score and loses in all three rows
    assert MC.LOGPS.index(max(MC.LOGPS)) == 3 and all(w != 3 for _, _, _, w in MC.WORKED)
    assert m.consensus_utilities(MC.HYPS, MC.LOGPS, df, 4) == MC.WORKED[0][2]                     # the defaults: CIDEr only, uniform


def test_the_definition_term_by_term():
    """U_i from cider_d / rouge_l called exactly as the definition writes them, j ascending"""
    m = _m()
    df = m.document_frequency(REFS)
    H, s, wc, wr, alpha = MC.HYPS, MC.LOGPS, 0.5, 0.5, 1.0
    q = [math.exp(alpha * (x - max(s))) for x in s]
    for i in range(len(H)):
        num = den = 0.0
        for j in range(len(H)):
            if j != i:
                gain = wc * m.cider_d([[H[j]]], [H[i]], df=df, n_images=4, sigma=6.0)[0] + wr * m.rouge_l([H[j]], H[i])
                num += q[j] * gain; den += q[j]
        assert m.consensus_utilities(H, s, df, 4, (wc, wr), alpha)[i] == num / den


def test_edge_cases():
    m = _m()
    df = m.document_frequency(TWO)
    u = lambda hyps, **kw: m.consensus_utilities(hyps, [-1.0 - i for i in range(len(hyps))], df, 2, **kw)
    assert u([]) == [] and u([[1, 2]]) == [0.0] and u([[1, 2]], reward=(0.5, 0.5), alpha=2.0) == [0.0]          # F = 1: nothing to agree with
    # two identical hypotheses: an exact tie, the first wins; cider of a sentence with itself: orders 1 and 2 at 1 -> 10 * 2 / 4
    two = u([[1, 2], [1, 2]])
    assert two[0] == two[1] and abs(two[0] - 5.0) <= 1e-12 and two.index(max(two)) == 0
    three = u([[1, 2], [1, 2], [1, 2]], reward=(0.5, 0.5))
    assert len(set(three)) == 1 and abs(three[0] - (0.5 * 5.0 + 0.5 * 1.0)) <= 1e-12 and three.index(max(three)) == 0
    # weighted votes (alpha > 0) for the same gain: the same value up to the roundings of the weighted mean
    assert all(abs(x - three[0]) <= 1e-12 for x in u([[1, 2], [1, 2], [1, 2]], reward=(0.5, 0.5), alpha=1.0))
    # an empty hypothesis scores 0 and gives the others 0
    e = u([[], [1, 2], [1, 2]], reward=(0.5, 0.5))
    assert e[0] == 0.0 and abs(e[1] - 0.5 * (0.0 + 0.5 * 5.0 + 0.5 * 1.0)) <= 1e-12 and e[1] == e[2]
    # a one-word hypothesis: len_s = 0, no bigram; against [1, 2]: unigram cosine 1 / sqrt(2), one bigram position apart
    one = u([[1], [1, 2]])
    pen = math.exp(-1 / 72)
    assert abs(one[0] - 10 * (1 / math.sqrt(2)) * pen / 4) <= 1e-12 and abs(one[1] - one[0]) <= 1e-12
    r = u([[1], [1, 2]], reward=(0.0, 1.0))
    assert abs(r[0] - 2.44 * 1.0 * 0.5 / (0.5 + 1.44 * 1.0)) <= 1e-12 and abs(r[1] - 2.44 * 0.5 * 1.0 / (1.0 + 1.44 * 0.5)) <= 1e-12
    # alpha = 0 is the uniform mean of the gains, whatever the raw scores are
    hyps = [[1, 2, 3], [1, 2], [3, 4], [1, 1, 2]]
    uni = m.consensus_utilities(hyps, [0.0] * 4, df, 2, (0.5, 0.5), 0.0)
    assert uni == m.consensus_utilities(hyps, [-9.0, -1.0, -5.0, -2.0], df, 2, (0.5, 0.5), 0.0)
    for i in range(4):
        gains = [0.5 * m.cider_d([[hyps[j]]], [hyps[i]], df=df, n_images=2)[0] + 0.5 * m.rouge_l([hyps[j]], hyps[i]) for j in range(4) if j != i]
        assert abs(uni[i] - sum(gains) / 3) <= 1e-12
    # a weight of 0 skips its term; both weights non-zero is the weighted sum of the two
    c, g = m.consensus_utilities(hyps, None, df, 2, (1.0, 0.0)), m.consensus_utilities(hyps, None, df, 2, (0.0, 1.0))
    both = m.consensus_utilities(hyps, None, df, 2, (0.25, 2.0))
    assert all(abs(b - (0.25 * x + 2.0 * y)) <= 1e-12 for b, x, y in zip(both, c, g))
    # a sharp alpha: every vote but the best-scored hypothesis's vanishes
    sharp = m.consensus_utilities(hyps, [-9.0, -1.0, -5.0, -2.0], df, 2, (0.0, 1.0), 50.0)
    assert abs(sharp[0] - m.rouge_l([hyps[1]], hyps[0])) <= 1e-12
    for bad in (dict(reward=(0.0, 0.0)), dict(reward=(-1.0, 1.0)), dict(alpha=-0.5), dict(alpha=float("inf")), dict(reward=(float("nan"), 1.0))):
        with pytest.raises(ValueError):
            u(hyps, **bad)


def test_generated_beams_have_the_cases_they_are_meant_to_have():
    """mbr_cases.beams has the cases it is meant to have: every count 0..K, an empty, a one-word and a full-width hypothesis, identical
    hypotheses that tie.  (That at least 3/4 of its images keep best and second best >= 1e-6 apart is asserted, from host values alone,
    in test_gpu_mbr.py, where the K = 32 reference is computed anyway.)"""
    m = _m()
    df = m.document_frequency(MC.corpus_refs())
    for K, W in MC.SHAPES:
        hyps, logps = MC.beams(K, W)
        assert sorted(set(len(h) for h in hyps)) == list(range(K + 1)) and {0, 1, W} <= {len(c) for h in hyps for c in h}
        assert all(len(h) <= K and all(len(c) <= W for c in h) for h in hyps)
    hyps, logps = MC.beams(5, 10)
    for reward, alpha in MC.REWARDS:
        us = [m.consensus_utilities(h, s, df, 37, reward, alpha) for h, s in zip(hyps, logps)]
        assert us[6][0] > 0.0 and all(abs(x - us[6][0]) <= 1e-12 for x in us[6])
        assert alpha != 0.0 or len(set(us[6])) == 1                     # uniform votes: the identical hypotheses tie exactly
        assert all(0.0 <= x for u in us for x in u)


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
    for name in ("sat_beam_hypotheses", "sat_caption_mbr", "sat_beam_select_at"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS and re.search(r"\bint %s\s*\(" % name, code), name
    assert "#define SAT_MBR_MAX_HYPS 32" in header and _lib.MBR_MAX_HYPS == 32
    assert _lib.RESCORE == {None: 0, "NONE": 0, "LN": 1, "WR": 2, "BAR": 3}                      # "MBR" never reaches sat_beam_select
    lib.sat_abi_version.restype = ctypes.c_int
    assert lib.sat_abi_version() == 23 and "#define SAT_HIP_ABI_VERSION 23" in header          # symbols were added, nothing existing changed


def test_argument_checks_come_before_any_launch(lib):
    """null pointers, sizes beyond the limits, refused capacities, weights and alpha return SAT_EINVAL (1) with text"""
    from sat_amd import _lib
    p = 4096                                                            # a non-null address: never dereferenced on the host
    err = lambda: lib.sat_last_error()
    hy = lambda **kw: lib.sat_beam_hypotheses(kw.get("tok_in", p), kw.get("prev", p), kw.get("cnt", p), kw.get("step", p), kw.get("row", p), kw.get("B", 2),
                                              kw.get("K", 4), kw.get("S", 9), 0, kw.get("out", p), kw.get("len", p), None)
    for null in ("tok_in", "prev", "cnt", "step", "row", "out", "len"):
        assert hy(**{null: None}) == 1 and b"beam_hypotheses: null" in err(), null
    for zero in ("B", "K", "S"):
        assert hy(**{zero: 0}) == 1 and b"non-positive" in err(), zero
    assert hy(S=_lib.CAPTION_MAX_LEN) == 1 and b"over the limit" in err()
    mb = lambda **kw: lib.sat_caption_mbr(kw.get("tok", p), kw.get("len", p), kw.get("cnt", p), kw.get("logp", p), kw.get("B", 2), kw.get("K", 5),
                                          kw.get("W", 10), kw.get("table", p), kw.get("cap", 64), kw.get("N", 10), kw.get("sigma", 6.0), kw.get("wc", 1.0),
                                          kw.get("wr", 0.0), kw.get("alpha", 0.0), kw.get("util", p), kw.get("win", p), None)
    for null in ("tok", "len", "cnt", "table", "util", "win"):
        assert mb(**{null: None}) == 1 and b"caption_mbr: null" in err(), null
    assert mb(logp=None, alpha=1.0) == 1 and b"hyp_logp" in err()
    for zero in ("B", "K", "W"):
        assert mb(**{zero: 0}) == 1 and b"non-positive" in err(), zero
    assert mb(K=_lib.MBR_MAX_HYPS + 1) == 1 and b"over the limits" in err()
    assert mb(W=_lib.CAPTION_MAX_LEN + 1) == 1 and b"over the limits" in err()
    for cap in (0, 48, -64):
        assert mb(cap=cap) == 1 and b"power of two" in err(), cap
    assert mb(N=0) == 1 and b"n_images" in err()
    assert mb(sigma=0.0) == 1 and b"sigma" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert mb(wc=bad) == 1 and b"weights" in err(), bad
        assert mb(wr=bad) == 1 and b"weights" in err(), bad
        assert mb(alpha=bad) == 1 and b"alpha" in err(), bad
    assert mb(wc=0.0, wr=0.0) == 1 and b"both weights" in err()
    at = lambda **kw: lib.sat_beam_select_at(kw.get("tok_in", p), kw.get("prev", p), kw.get("cnt", p), kw.get("step", p), kw.get("row", p),
                                             kw.get("score", p), kw.get("hist", p), kw.get("pick", p), kw.get("pick_score", None), kw.get("B", 2),
                                             kw.get("K", 4), kw.get("S", 9), kw.get("L", 12), 0, kw.get("tok", p), kw.get("len", p), kw.get("cs", p),
                                             kw.get("raw", p), kw.get("st", p), kw.get("alpha", None), None)
    for null in ("tok_in", "prev", "cnt", "step", "row", "score", "pick", "tok", "len", "cs", "raw", "st"):
        assert at(**{null: None}) == 1 and b"beam_select_at: null" in err(), null
    assert at(alpha=p, hist=None) == 1 and b"alpha_hist" in err()
    for zero in ("B", "K", "S"):
        assert at(**{zero: 0}) == 1 and b"non-positive" in err(), zero
    assert at(alpha=p, L=0) == 1 and b"non-positive" in err()
    assert at(S=_lib.CAPTION_MAX_LEN) == 1 and b"over the limit" in err()


class _Corpus:
    """what check_mbr reads of a ReferenceCorpus"""

    def __init__(self, images=5, overflow=False):
        self.images, self.overflow, self.reads, self._checked_images = images, overflow, 0, None

    def check(self):
        from sat_amd import _lib
        self.reads += 1
        if self.overflow:
            raise _lib.SatHipError("ReferenceCorpus: the table overflowed")
        self._checked_images = self.images
        return self


def test_python_refusals_touch_no_gpu():
    import torch
    import sat_amd  # noqa: F401
    from sat_amd import constraints, evaluation as E, model as M
    ok = _Corpus()
    chk = lambda **kw: constraints.check_mbr(kw.get("method", "MBR"), kw.get("corpus", ok), kw.get("reward", (1.0, 0.0)), kw.get("alpha", 0.0),
                                             kw.get("beamk", 5), kw.get("V", 6400), kw.get("S", 32))
    assert chk() == (1.0, 0.0, 0.0) and chk(reward=[0.5, 0.5], alpha=1) == (0.5, 0.5, 1.0)
    assert ok.reads == 1                                                 # checked once per state, not once per batch
    for method in (None, "LN", "WR", "BAR"):
        assert chk(method=method, corpus=None, beamk=64, V=10 ** 6) is None          # the reference rules never look at the keywords
    for bad, text in ((dict(corpus=None), "mbr_corpus"), (dict(corpus=_Corpus(images=0)), "no image"), (dict(corpus=_Corpus(overflow=True)), "overflow"),
                      (dict(beamk=33), "beamk"), (dict(beamk=0), "beamk"), (dict(V=65536), "vocab_size"), (dict(S=0), "max_gen_length"),
                      (dict(S=128), "max_gen_length"), (dict(reward=(0.0, 0.0)), "both weights"), (dict(reward=(-1.0, 1.0)), "finite"),
                      (dict(alpha=-1.0), "finite"), (dict(alpha=float("nan")), "finite"), (dict(reward=(1.0,)), "mbr_reward"),
                      (dict(reward=None), "mbr_reward")):
        with pytest.raises(ValueError, match=text):
            chk(**bad)
    # through the public calls, on the CPU: the ValueError comes before anything needs a device
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=83, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40)
    dec = M.SATDecoder(hp).eval()
    ann = torch.zeros(2, 12, 32)
    with pytest.raises(ValueError, match="mbr_corpus"):
        dec.beam_decode_batched(ann, (3, 4), beamk=4, max_gen_length=9, rescore_method="MBR")
    with pytest.raises(ValueError, match="beamk"):
        dec.beam_decode_batched(ann, (3, 4), beamk=33, max_gen_length=9, rescore_method="MBR", mbr_corpus=ok)
    with pytest.raises(ValueError, match="overflow"):
        dec.beam_decode_batched(ann, (3, 4), beamk=4, max_gen_length=9, rescore_method="MBR", mbr_corpus=_Corpus(overflow=True))
    with pytest.raises(ValueError, match="batched"):
        dec.beam_decode(ann, (3, 4), beamk=4, max_gen_length=9, rescore_method="MBR")
    buffers = dict(tok_in=torch.zeros(11, 2, 4, dtype=torch.int32), alpha_hist=torch.zeros(10, 2, 4, 12))
    with pytest.raises(ValueError, match="mbr_corpus"):
        E.select_hypotheses(buffers, 0, "MBR")
    with pytest.raises(ValueError, match="rescore_method"):
        E.select_hypotheses(buffers, 0, "XYZ")


#: evaluation.draw_decode_params from np.random.RandomState(3) over NOTEBOOK_SPACE, recorded with the code before "MBR" existed
RECORDED = [
    {"beamk": 5, "temperature": 0.7353624400054954, "sample_method": "multinomial", "decoder_noise": 0.0, "rescore_method": "LN", "rescore_reward": 0.6849300068436512},
    {"beamk": 20, "temperature": 1.1464734771738274, "sample_method": "beam", "decoder_noise": 0.0, "rescore_method": "BAR", "rescore_reward": 0.6879097173246853},
    {"beamk": 5, "temperature": 0.8239441486130177, "sample_method": "beam", "decoder_noise": 0.0, "rescore_method": "LN", "rescore_reward": 1.0863765569099288},
    {"beamk": 20, "temperature": 0.9284166121973555, "sample_method": "beam", "decoder_noise": 0.0, "rescore_method": "LN", "rescore_reward": 0.7949410978535827}]


class _StubModel:
    """fixed statistics (CPU tensors); scored against a corpus when one is passed, as tests/test_consensus.py's"""

    def __init__(self):
        self.calls = []

    def val_batch_stats(self, batch, **decode):
        import torch
        from sat_amd.evaluation import CaptionStats
        self.calls.append(decode)
        counts = torch.tensor([8, 5, 3, 2, 10, 9, 8, 7, 10, 11, 18, 34], dtype=torch.int64) * (1 + batch)
        consensus = torch.tensor([2.5, 1.25], dtype=torch.float64) if decode.get("corpus") is not None else None
        return CaptionStats(counts, torch.tensor(1.5, dtype=torch.float64), torch.tensor(6.0, dtype=torch.float64), 2, consensus)


def test_random_search_draws_are_the_recorded_ones():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model = _StubModel()
    rows = E.random_search(model, [0, 1, 2, 3], trials=4, seed=3)
    assert [{k: r[k] for k in E.HEADERS[:6]} for r in rows] == RECORDED
    assert all(list(r) == E.HEADERS + [k + "_corpus" for k in E.METRIC_KEYS] for r in rows)
    assert all(not any(k.startswith("mbr_") for k in c) for c in model.calls)                    # without "MBR" in the space nothing travels
    # "MBR" in the space: only with a corpus; the trial carries the method and the three keywords
    space = dict(E.NOTEBOOK_SPACE, rescore_methods=["MBR"])
    with pytest.raises(ValueError, match="mbr_corpus"):
        E.random_search(model, [0, 1], trials=1, space=space, seed=3)
    corpus = object()
    for kw, want_corpus in ((dict(mbr_corpus=corpus), False), (dict(corpus=corpus), True)):
        model.calls.clear()
        out = E.random_search(model, [0, 1], trials=2, space=space, seed=3, mbr_reward=(0.5, 0.5), mbr_alpha=1.0, **kw)
        assert all(r["rescore_method"] == "MBR" for r in out)
        assert all(c["rescore_method"] == "MBR" and c["mbr_corpus"] is corpus and c["mbr_reward"] == (0.5, 0.5) and c["mbr_alpha"] == 1.0 for c in model.calls)
        assert all(("corpus" in c) == want_corpus for c in model.calls)
