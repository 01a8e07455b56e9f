"""GPU: one search descriptor ("One search descriptor").  Every family of the batched search through its entry point from
before the descriptor and through sat_beam_search: the same bits in every output buffer, the same launches, a workspace of exactly the
queried size; and the Python path (``_beam_search_device`` of a decoder and of an ensemble) against the raw call.
Shapes of test_gpu_constrained_search.py cut down: V = 83, L = 12, D = 32, A = 16, m = 24, n = 40, 3 images x 4 beams, max_gen_length = 6,
temperatures [1.0, 0.7]."""
import ctypes as C

import pytest
import torch

import beam_search_desc_cases as BC

pytestmark = pytest.mark.gpu

V, B, K, S = 83, 3, 4, 6
TEMPS = [1.0, 0.7]
GUARD = 256
_cache = {}


def _member(layers=1, seed=None, Lc=12, **over):
    """(decoder, hparams, annotations (3, Lc, D)) on the GPU, built once"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    key = (layers, seed, Lc, tuple(sorted(over.items())))
    if key not in _cache:
        hp = O.default_hparams(**dict(dict(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, decoder_layers=layers), **over))
        torch.manual_seed(3 + layers if seed is None else seed)
        dec = M.SATDecoder(hp).cuda().eval()
        _cache[key] = (dec, hp, torch.from_numpy(prng.uniform((B, Lc, int(hp.encoder_dim)), 55 + Lc, 0.0, 1.0)).cuda())
    return _cache[key]


def _dims(dec, hp, ann):
    from sat_amd import decoder as Dk
    _, Lc, D = ann.shape
    return Dk.decoder_dims(B, K, 2, Lc, D, 16, 24, int(hp.decoder_dim), V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))


def _gumbel():
    g = torch.Generator().manual_seed(5)
    return (-torch.log(-torch.log(torch.rand(S + 1, B * K, 3, generator=g).clamp_(1e-9, 1 - 1e-7)))).cuda().contiguous()


#: name -> (old entry, LSTM layers, the Python keywords of the family)
CASES = {
    "batched": ("batched", 2, dict()),
    "sampled": ("sampled", 1, dict(sample_method="topk", sample_topk=3, seed=1)),                    # + the Gumbel table
    "constrained": ("constrained", 1, dict(prefix=[[], [20], [21, 22, 23]], banned=[30, 31])),
    "topg": ("constrained", 1, dict(topg=2)),
    "history": ("history", 1, dict(no_repeat_ngram=2, repetition_penalty=1.3)),
    "groups": ("groups", 1, dict(beam_groups=2, diversity_penalty=0.5)),
    "required": ("required", 1, dict(required=[[24, 25], [], [26, 27]])),
    "ensemble": ("ensemble", 1, dict(no_repeat_ngram=2, banned=[30])),
}


def _case(name):
    """(old entry, the parts of the raw calls, Lc of the attention maps, a thunk that runs the Python path)"""
    from sat_amd import _lib as L, constraints as Cn, ensemble as En
    entry, layers, kw = CASES[name]
    if name == "sampled":
        kw = dict(kw, gumbel=_gumbel())
    opt = Cn.SearchOptions(**kw)
    dec, hp, ann = _member(layers)
    con, hist, grp, req = opt.resolve(hp.vocab_stoi, V, B, K, S)
    keep = [opt]
    structs = {}
    for key, part in (("con", con), ("req", req)):
        if part is not None:
            structs[key], tensors = part.device_struct("cuda")
            keep.append(tensors)
    for key, part in (("hist", hist), ("grp", grp)):
        if part is not None:
            structs[key] = part.device_struct()
    if name == "sampled":
        structs["smp"] = L.BeamSampling(method=L.SAMPLE_METHODS["topk"], sample_topk=3, seed=1, gumbel=kw["gumbel"].data_ptr())
    ids = [int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")]
    if entry != "ensemble":
        w, tens = dec._params_struct()
        parts = BC.Parts(dims=_dims(dec, hp, ann), w=w, ann=ann.data_ptr(), beamk=K, S=S, temps=TEMPS, ids=ids, keep=keep + [tens], **structs)
        return entry, parts, ann.shape[1], lambda: dec._beam_search_device(ann, K, S, TEMPS, options=opt)
    other, hpo, anno = _member(2, seed=11, Lc=6, encoder_dim=48, decoder_dim=56, deep_output=True)          # another L, D, n, depth and output
    model = En.Ensemble([dec, other], [0.6, 0.4], "geometric")
    ens = L.BeamEnsemble(members=2, combine=L.ENSEMBLE_COMBINE["geometric"])
    for i, (m, h, a, wt) in enumerate(((dec, hp, ann, model.weights[0]), (other, hpo, anno, model.weights[1]))):
        d, (w, tens) = _dims(m, h, a), m._params_struct()
        keep += [d, w, tens]
        ens.dims[i], ens.params[i], ens.ann[i], ens.weight[i] = C.pointer(d), C.pointer(w), a.data_ptr(), wt
    parts = BC.Parts(ens=ens, beamk=K, S=S, temps=TEMPS, ids=ids, keep=keep, **structs)
    return entry, parts, ann.shape[1], lambda: model._beam_search_device([ann, anno], K, S, TEMPS, options=opt)


def _old_workspace_bytes(lib, entry, p):
    if entry == "ensemble":
        return lib.sat_beam_search_ensemble_workspace_bytes(C.byref(p.ens), K, S)
    d = C.byref(p.dims)
    return {"batched": lambda: lib.sat_beam_search_workspace_bytes(d, K), "sampled": lambda: lib.sat_beam_search_workspace_bytes(d, K),
            "constrained": lambda: lib.sat_beam_search_constrained_workspace_bytes(d, K, p.con.topg),
            "history": lambda: lib.sat_beam_search_history_workspace_bytes(d, K, 0, S),
            "groups": lambda: lib.sat_beam_search_groups_workspace_bytes(d, K, p.grp.groups, S),
            "required": lambda: lib.sat_beam_search_required_workspace_bytes(d, K, S, p.req.max_required)}[entry]()


def _raw(entry, p, Lc, new):
    """the search on zeroed buffers through the old entry or through sat_beam_search: (buffers, {profiled scope: launches}, workspace,
    queried bytes).  The new call's workspace is the queried size followed by GUARD bytes of 0xA5."""
    from sat_amd import _lib as L
    lib = L.lib()
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(tok_in=torch.zeros(S + 2, B, K, **i32), prev_row=torch.zeros(S + 2, B, K, **i32), alpha_hist=torch.zeros(S + 1, B, K, Lc, **f32),
             fin_count=torch.zeros(B, **i32), fin_step=torch.zeros(B, K, **i32), fin_row=torch.zeros(B, K, **i32), fin_score=torch.zeros(B, K, **f32),
             fin_mean=torch.zeros(B, K, **f32))
    if p.req is not None:
        o["req_met"] = torch.zeros(B, **i32)
    if new:
        nbytes = lib.sat_beam_search_desc_workspace_bytes(C.byref(BC.descriptor(L, p)))
    else:
        nbytes = _old_workspace_bytes(lib, entry, p)
    assert nbytes > 0, lib.sat_last_error().decode()
    ws = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0xA5
    outs = [L.ptr(o[k]) for k in BC.OUTPUTS]
    torch.cuda.synchronize()
    L.profile_start()
    if new:
        rc = BC.new_call(L, p, outs, L.ptr(o.get("req_met")), L.ptr(ws), nbytes, L.stream_ptr())
    else:
        rc = BC.old_call(lib, entry, p, outs, L.ptr(o.get("req_met")), L.ptr(ws), nbytes, L.stream_ptr())
    torch.cuda.synchronize()
    launches = {e["name"]: e["launches"] for e in L.profile_stop()}
    L.check(rc, "sat_beam_search" if new else "sat_beam_search_" + entry)
    return o, launches, ws, nbytes


@pytest.mark.parametrize("name", list(CASES))
def test_descriptor_runs_what_the_old_entry_runs(name):
    """the same bits in every buffer, no launch gained or lost, the queried workspace is enough (the guard behind it is intact), and the
    Python path returns what the raw call leaves"""
    entry, parts, Lc, python_path = _case(name)
    want, launches_old, _, bytes_old = _raw(entry, parts, Lc, new=False)
    got, launches_new, ws, nbytes = _raw(entry, parts, Lc, new=True)
    assert int(want["fin_count"].min()) >= 1 and set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (name, k)
    assert launches_new == launches_old and sum(launches_old.values()) > 0, (name, launches_old, launches_new)
    assert nbytes <= bytes_old and bool((ws[nbytes:] == 0xA5).all()), name
    if name == "required":                                   # the words the search was given are met where the vocabulary allows
        assert got["req_met"].tolist()[1] == 0 and int(got["req_met"].max()) <= 2
    o = python_path()
    torch.cuda.synchronize()
    assert set(o) == set(got) | {"ws"} and o["ws"].numel() == nbytes
    for k in got:
        assert o[k].dtype == got[k].dtype and torch.equal(o[k], got[k]), (name, k)
