"""GPU: the constrained batched search ("Constrained search"): forced prefix, top-g clipping, banned ids.
Shapes of test_batched_beam_search_equals_the_per_image_loop: V = 83 (every kernel's tail), 9 images x 4 beams (rows die at different
steps), L = 12, max_gen_length = 9, temperatures [1.0, 0.7], one and two LSTM layers."""
import ctypes as C
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu

V, S, HW = 83, 9, (3, 4)
TEMPS = [1.0, 0.7]
PLENS = [0, 1, 3, 0, 2, 9, 1, 0, 4]
#: seeds of test 4, chosen on the CPU: the reference search alone keeps every pick >= 1e-3 (relative) away from the next candidate
ORACLE_SEEDS = {1: 246, 2: 115}
_cache = {}


def _setup(layers, seed=None):
    """(decoder, hparams, annotations (9, 12, 32)); one model per layer count and seed, built once"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    key = (layers, seed)
    if key not in _cache:
        hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, decoder_layers=layers)
        torch.manual_seed(3 + layers if seed is None else seed)
        dec = M.SATDecoder(hp).cuda().eval()
        _cache[key] = (dec, hp, torch.from_numpy(prng.uniform((9, 12, 32), 55, 0.0, 1.0)).cuda())
    return _cache[key]


def _plain(layers, beamk, **kw):
    """the unconstrained batched search, computed once per case and left unchanged"""
    key = ("plain", layers, beamk, tuple(sorted(kw.items())))
    if key not in _cache:
        dec, _, ann = _setup(layers)
        _cache[key] = dec.beam_decode_batched(ann, HW, beamk=beamk, max_gen_length=S, temperature=TEMPS, **kw)
    return _cache[key]


def _flat(x):
    return [v for e in x for v in (e if isinstance(e, list) else [e])]


def _close(a, b, tol):
    """captions and list order identical; scores, perplexities and maps within tol (relative for the scalars)"""
    assert a[0] == b[0]
    for i in (1, 3):
        for u, v in zip(_flat(a[i]), _flat(b[i])):
            assert abs(u - v) <= tol * max(1.0, abs(u)), (i, u, v)
    for u, v in zip(_flat(a[2]), _flat(b[2])):
        assert u.shape == v.shape and float((u.cpu() - v.cpu()).abs().max()) <= tol


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    assert all(torch.equal(u, v) for u, v in zip(_flat(a[2]), _flat(b[2])))


def _prefixes(lens, skip=()):
    """arbitrary ordinary words (never a special id, none of ``skip``), lens[b] of them for image b"""
    ok = [t for t in range(1, V - 3) if t not in skip]
    return [[ok[(7 * b + 3 * i) % len(ok)] for i in range(n)] for b, n in enumerate(lens)]


def _raw(dec, hp, ann, K, entry, smp=None, con=None):
    """one of the C entry points on zeroed buffers: {tok_in, prev_row, alpha_hist, fin_*}"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    B, Lc, D = ann.shape
    dims = Dk.decoder_dims(B, K, 2, Lc, D, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
    w, keep = dec._params_struct()
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(tok_in=torch.zeros(S + 2, B, K, **i32), prev_row=torch.zeros(S + 2, B, K, **i32), alpha_hist=torch.zeros(S + 1, B, K, Lc, **f32),
             fin_count=torch.zeros(B, **i32), fin_step=torch.zeros(B, K, **i32), fin_row=torch.zeros(B, K, **i32), fin_score=torch.zeros(B, K, **f32),
             fin_mean=torch.zeros(B, K, **f32))
    tarr = (C.c_float * len(TEMPS))(*TEMPS)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    outs = [L.ptr(o[k]) for k in ("tok_in", "prev_row", "alpha_hist", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean")]
    smp_p = C.byref(smp) if smp is not None else None
    if entry == "sampled":
        nbytes = lib.sat_beam_search_workspace_bytes(C.byref(dims), K)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        L.check(lib.sat_beam_search_sampled(C.byref(dims), C.byref(w), L.ptr(ann), K, S, tarr, len(TEMPS), ids, smp_p, *outs, L.ptr(ws), nbytes, L.stream_ptr()),
                "sat_beam_search_sampled")
    else:
        nbytes = lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, con.topg if con is not None else 0)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        L.check(lib.sat_beam_search_constrained(C.byref(dims), C.byref(w), L.ptr(ann), K, S, tarr, len(TEMPS), ids, smp_p, C.byref(con) if con is not None else None,
                                                *outs, L.ptr(ws), nbytes, L.stream_ptr()), "sat_beam_search_constrained")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("layers", [1, 2])
def test_no_constraint_is_todays_search_bit_for_bit(layers):
    """1. NULL / empty constraints, and a prefix array whose every length is 0 (which does take the constrained kernels), against
    sat_beam_search_sampled: every back-trace buffer equal.  Beams 1 and 4, and once the sampled "topk" search on a Gumbel table."""
    from sat_amd import _lib as L
    dec, hp, ann = _setup(layers)
    B = ann.shape[0]
    pre = torch.tensor(_prefixes([3] * B), dtype=torch.int32, device="cuda")
    zero_len = torch.zeros(B, dtype=torch.int32, device="cuda")
    runs = [(1, None), (4, None)]
    if layers == 2:
        g = torch.Generator().manual_seed(5)
        gum = (-torch.log(-torch.log(torch.rand(S + 1, B * 4, 3, generator=g).clamp_(1e-9, 1 - 1e-7)))).cuda().contiguous()
        runs.append((4, L.BeamSampling(method=2, sample_topk=3, seed=1, gumbel=gum.data_ptr())))
    for K, smp in runs:
        want = _raw(dec, hp, ann, K, "sampled", smp)
        assert int(want["fin_count"].min()) >= 1
        for con in (None, L.BeamConstraints(), L.BeamConstraints(max_prefix=3, prefix=pre.data_ptr(), prefix_len=zero_len.data_ptr())):
            got = _raw(dec, hp, ann, K, "constrained", smp, con)
            for k in want:
                assert torch.equal(got[k], want[k]), (K, smp is not None, con is not None and con.max_prefix, k)


@pytest.mark.parametrize("layers", [1, 2])
def test_topg_at_least_beamk_is_plain_beam_search_bit_for_bit(layers):
    """2. the union of the rows' top K holds the global top K under the same tie order"""
    dec, _, ann = _setup(layers)
    for rm in ("LN", "BAR"):
        want = _plain(layers, 4, rescore_method=rm, return_all=True)
        for g in (4, 7):
            _same(dec.beam_decode_batched(ann, HW, beamk=4, max_gen_length=S, temperature=TEMPS, rescore_method=rm, return_all=True, topg=g), want)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("g", [1, 2])
def test_topg_equals_the_per_image_loop(layers, g):
    """3. captions and list order identical, values within 1e-5 (the batched-vs-loop rule); topg = 1: no two kept hypotheses of a
    step share a parent"""
    dec, _, ann = _setup(layers)
    kw = dict(beamk=4, max_gen_length=S, temperature=TEMPS, rescore_method="BAR", return_all=True, topg=g)
    got = dec.beam_decode_batched(ann, HW, **kw)
    _close(dec.beam_decode(ann, HW, **kw), got, 1e-5)
    assert got[0] != _plain(layers, 4, rescore_method="BAR", return_all=True)[0]          # the clipping changes this search
    if g == 1:
        o = {k: v.cpu() for k, v in dec._beam_search_device(ann, 4, S, TEMPS, "beam", 3, None, None, None, None, False, topg=1).items()}
        for b in range(ann.shape[0]):
            fin = [(int(o["fin_step"][b, f]), int(o["fin_row"][b, f])) for f in range(int(o["fin_count"][b]))]
            for s in range(1, S + 1):
                parents = [r for st, r in fin if st == s]
                if s < S:                               # live rows of step s + 1 (a fed token is never <PAD> = 0)
                    parents += o["prev_row"][s + 1, b][o["tok_in"][s + 1, b] != 0].tolist()
                assert len(set(parents)) == len(parents), (b, s, parents)


@pytest.mark.parametrize("layers", [1, 2])
def test_topg_against_the_cpu_reference_search(layers):
    """4. softmax is monotone, so the reference's "topk" branch with a deterministic pick IS top-g clipping.  Captions identical,
    values within 1e-4 (the GPU-vs-CPU bound); the hook proves no pick of the reference was a near-tie."""
    from oracle import sat_oracle as O
    dec, hp, ann = _setup(layers, seed=ORACLE_SEEDS[layers])
    sd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    ann_img = ann.cpu().reshape(9, 3, 4, 32).permute(0, 3, 1, 2).contiguous()
    gaps = []

    def pick(p, k):
        s = torch.sort(p, descending=True).values
        if len(s) > k:
            gaps.append(float((s[k - 1] - s[k]) / s[k - 1]))
        return torch.topk(p, k).indices

    kw = dict(beamk=4, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
    with torch.no_grad():
        want = O.beam_search(sd, hp, ann_img, sample_method="topk", sample_topk=2, multinomial=pick, **kw)
    print("smallest relative gap of the reference's picks: %.3e over %d picks" % (min(gaps), len(gaps)))
    assert min(gaps) >= 1e-3
    got = dec.beam_decode_batched(ann, HW, topg=2, **kw)
    want = (want[0], want[1], [[a.reshape(-1, *HW) for a in al] for al in want[2]], want[3])
    _close(want, got, 1e-4)


@pytest.mark.parametrize("layers", [1, 2])
def test_greedy_prefix_identity(layers):
    """5. beam 1: forcing the first words of the unconstrained caption changes nothing, bit for bit"""
    dec, hp, ann = _setup(layers)
    want = _plain(layers, 1, rescore_method="LN")
    special = {int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")}
    prefix = [c[:min([p, len(c)] + [i for i, t in enumerate(c) if t in special])] for c, p in zip(want[0], PLENS)]
    assert sum(len(p) > 0 for p in prefix) >= 5 and len({len(p) for p in prefix}) >= 4
    _same(dec.beam_decode_batched(ann, HW, beamk=1, max_gen_length=S, temperature=TEMPS, rescore_method="LN", prefix=prefix), want)


@pytest.mark.parametrize("layers", [1, 2])
def test_prefix_of_mixed_lengths_equals_the_per_image_loop(layers):
    """6. beam 4, prefix lengths 0..9 in one batch"""
    dec, _, ann = _setup(layers)
    prefix = _prefixes(PLENS)
    kw = dict(beamk=4, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, prefix=prefix)
    got = dec.beam_decode_batched(ann, HW, **kw)
    _close(dec.beam_decode(ann, HW, **kw), got, 1e-5)
    for b, caps in enumerate(got[0]):
        assert all(c[:len(prefix[b])] == prefix[b] for c in caps), (b, caps)
    assert got[0][5] == [prefix[5]] * 4                 # P_b = max_gen_length: the K rows are cut at the limit
    plain = _plain(layers, 4, rescore_method="LN", return_all=True)
    for b in (0, 3, 7):                                 # P_b = 0: that image's search is the plain one
        assert got[0][b] == plain[0][b] and got[1][b] == plain[1][b]


def test_string_prefix_through_sat_caption():
    """6. a string prefix is split and looked up; one prefix is broadcast to every image"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    hp = O.default_hparams(**over)
    hp.vocab_stoi.update({"a": 4, "photo": 9, "of": 2}); hp.vocab_itos.update({4: "a", 9: "photo", 2: "of"})
    torch.manual_seed(5)
    model = M.SAT(**vars(hp)).cuda()
    img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 41, 0.0, 1.0)).cuda()
    kw = dict(beamk=3, max_gen_length=7, rescore_method="LN", return_all=True)
    got = model.caption(img, prefix="a photo of", **kw)
    assert all(c[:3] == [4, 9, 2] for caps in got[0] for c in caps) and all(len(caps) == 3 for caps in got[0])
    _same(model.caption(img, prefix=[4, 9, 2], **kw), got)
    assert model.decode_seq(got[0][0][0])[:3] == ["a", "photo", "of"]


@pytest.mark.parametrize("layers", [1, 2])
def test_banned_ids_never_appear(layers):
    """7. no_unk and two more banned ids (the two commonest words of the plain search, so the ban bites), alone and together with
    top-g clipping and a prefix"""
    dec, hp, ann = _setup(layers)
    plain = _plain(layers, 4, rescore_method="LN", return_all=True)
    special = {int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")}
    common = [t for t, _ in Counter(t for caps in plain[0] for c in caps for t in c if t not in special).most_common(2)]
    assert len(common) == 2
    ban = set(common) | {int(hp.vocab_stoi["<UNK>"])}
    prefix = _prefixes(PLENS, skip=ban)
    for extra in (dict(), dict(topg=2, prefix=prefix)):
        kw = dict(beamk=4, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, banned=common, no_unk=True, **extra)
        got = dec.beam_decode_batched(ann, HW, **kw)
        assert not any(t in ban for caps in got[0] for c in caps for t in c)
        _close(dec.beam_decode(ann, HW, **kw), got, 1e-5)
        if extra:
            assert all(c[:len(prefix[b])] == prefix[b] for b, caps in enumerate(got[0]) for c in caps)


def test_evaluation_surface_takes_the_constraints():
    """8. val_batch_stats(...).metrics() against score_captions on caption(...), both with topg = 2 and no_unk: bleu / gleu exactly,
    cosine within max(2 e_torch, 1e-6) of the float64 value, perplexity 1e-6 relative (the rule of the unconstrained pair)"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16,
                decoder_dim=40, deep_output=True, val_beamk=3, val_max_len=7)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over))).cuda()
    img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 41, 0.0, 1.0)).cuda()
    caps, lengths = prng.captions(4, 3, 9, 60, 42, min_len=3)
    caps, lengths = torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="LN", rescore_reward=0.7, topg=2, no_unk=True)
    captions, _, _, ppl = model.caption(img, return_all=False, **kw)
    want = model.score_captions(captions, caps, lengths, ppl)
    assert want == model.val_batch((img, caps, lengths), **kw)
    got = model.val_batch_stats((img, caps, lengths), **kw).metrics()
    assert set(got) == set(want)
    for k in ("bleu1", "bleu2", "bleu3", "bleu4", "gleu"):
        assert got[k] == want[k], (k, got[k], want[k])
    E64 = model.embedding.weight.detach().cpu().double()
    c64 = []
    for i, h in enumerate(captions):
        cv = E64[torch.as_tensor(h, dtype=torch.long)].mean(0)
        rvs = [E64[caps[i][j][1:int(l)].cpu()].mean(0) for j, l in enumerate(lengths[i])]
        c64.append(max(float(((rv / rv.norm().clamp_min(1e-8)) * (cv / cv.norm().clamp_min(1e-8))).sum()) for rv in rvs))
    c64 = sum(c64) / len(c64)
    e_kernel, e_torch = abs(got["cosine_similarity"] - c64), abs(want["cosine_similarity"] - c64)
    print("cosine: e_kernel %.3e  e_torch %.3e" % (e_kernel, e_torch))
    assert e_kernel <= max(2 * e_torch, 1e-6)
    assert abs(got["perplexity"] - want["perplexity"]) <= 1e-6 * abs(want["perplexity"])
