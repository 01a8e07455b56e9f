"""GPU: the decoder's sub-module entry points and search primitives, each called on its own through the C ABI with raw pointers
(sat_colsum, sat_embedding_fwd / _bwd, sat_lstm_cell_fwd / _bwd, sat_deep_output_fwd / _bwd, sat_init_lstm_fwd / _bwd,
sat_doubly_stochastic_fwd / _bwd, sat_sigmoid_bwd, sat_topk, sat_beam_scores) against the float64 restatements of
tests/decoder_entry_ref.py, at the shapes of tests/decoder_entry_cases.py.  test_decoder_entry_ref.py proves without a GPU that the
restatements are torch's modules and that on these inputs they notice a dropped last row, column, occurrence or step.

Every allocation is the test's own: inputs are views inside NaN-filled buffers (NaN also in the padding columns of a strided
matrix), outputs and scratch are views inside canary buffers whose frames must be canaries afterwards.  Every entry point is called
twice on the same inputs and must give the same bits.

(a) exact: small integers (column sums, the embedding gradient, the row sums and the mean of the doubly stochastic term, the bias
    gradients of DeepOutput and InitLSTM, InitLSTM's df / dmean / dann with L a power of two, the sigmoid backward on dyadic y) must
    equal the float64 reference bit for bit whatever the order of the additions; the real-valued embedding gradient must equal an fp32
    chain in increasing row order bit for bit (the order include/sat_hip.h documents); the gather, the rows max_norm leaves alone,
    the dropout masks, top-k values and indices, -inf and masked positions are exact as well.
(b) bounded: reals within 1e-4 max(1, max|ref|) of float64 -- close() of test_gpu_modules.py and test_gpu_attention_forms.py; the
    worst error per entry point is printed ("Decoder entry points").  dalphas of the doubly stochastic term is of order
    1 / (N L), far below that bound's floor, so it is held to 8 * 2^-24 max|ref| as well: of its fp32 operations four round, once each.
    sat_beam_scores is held to the bound derived in tests/test_gpu_search_history.py, (ceil(V / 256) + 32) 2^-24 times the row's
    magnitude, the magnitude taken by that file's restatement over the entries of the row that are not -inf.
(c) the saturating LSTM variant: finite, |h| <= 1, within (b), and exact zeros in dgates wherever a gate came out as exactly 0 or 1
    (+-1 for the cell gate); the tiny variant: |h_new - float64| <= 4 |fp32 CPU nn.LSTMCell - float64| + 4e-7 in absolute terms."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import decoder_entry_cases as C
import decoder_entry_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAN = float("nan")
SEED = 0x5EEDC0DE12345


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)
    for entry in sorted(WORST):
        print("worst error of %s: %.3e" % (entry, WORST[entry]))


def _ids(cases, fn):
    return [pytest.param(i, c, id=fn(c)) for i, c in enumerate(cases)]


WORST = {}


def close(got, ref, what, entry):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    WORST[entry] = max(WORST.get(entry, 0.0), err / scale)
    print("%s: max|d| = %.3e (scale %.3g); worst of %s so far %.3e" % (what, err, scale, entry, WORST[entry]))
    assert err <= TOL * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, TOL)


def exact(got, ref, what):
    got = got.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    assert torch.equal(got, ref.float()), "%s: %d element(s) differ from the exact result" % (what, int((got != ref.float()).sum()))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def twice(run, what):
    """run() -> dict of device outputs; the same bits the second time"""
    a, b = run(), run()
    for k in a:
        if a[k] is not None:
            assert torch.equal(bits(a[k]), bits(b[k])), "%s: %s differs between two calls on the same inputs" % (what, k)
    return a


def framed(shapes, dtype=torch.float32):
    """name -> (whole, view) canary frames"""
    return {k: R.canary_framed(s, dtype) if s is not None else (None, None) for k, s in shapes.items()}


def frames_intact(fr, what):
    for k, (whole, _) in fr.items():
        if whole is not None:
            R.frame_intact(whole, "%s %s" % (what, k))


def views(fr):
    return {k: v for k, (_, v) in fr.items()}


def dev(fr, k, L):
    return L.ptr(fr[k][1]) if fr[k][1] is not None else None


def inputs(**tensors):
    """name -> device view inside a NaN frame (None stays None); the frames are kept alive next to the views"""
    keep, out = [], {}
    for k, t in tensors.items():
        if t is None:
            out[k] = None
        else:
            whole, view = R.nan_framed(t)
            keep.append(whole); out[k] = view
    out["_frames"] = keep
    return out


def inputs_intact(inp, what):
    for whole in inp["_frames"]:
        R.nan_frame_intact(whole, R.GUARD, what)


# ------------------------------------------------------------------ sat_colsum
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.COLSUM_CASES, C.colsum_id))
def test_colsum(L, i, c, dataset):
    lib = L.lib()
    rows, cols, ld = c["rows"], c["cols"], c["ld"]
    x = C.colsum_inputs(c, i, dataset)
    host = torch.full((rows, ld), NAN)
    host[:, :cols] = x
    xw, xd = R.nan_framed(host, c["off"])
    assert C.colsum_path(c) == c["path"] and (xd.data_ptr() % 16 == 0) == (c["off"] == 0)
    tag = "colsum %s %s" % (C.colsum_id(c), dataset)

    def run():
        fr = framed(dict(out=(cols,), scratch=(-(-rows // 256) * cols,)))
        L.check(lib.sat_colsum(L.ptr(xd), ld, rows, cols, dev(fr, "out", L), dev(fr, "scratch", L), L.stream_ptr()), "sat_colsum")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return dict(out=fr["out"][1])
    out = twice(run, tag)["out"]
    R.nan_frame_intact(xw, R.GUARD, tag)
    if dataset == "int":
        exact(out, R.colsum(x), tag)
    else:
        close(out, R.colsum(x), tag, "sat_colsum (%s)" % c["path"])


# ------------------------------------------------------------------ sat_embedding_bwd / sat_embedding_fwd
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.EMB_BWD_CASES, C.emb_bwd_id))
def test_embedding_gradient(L, i, c, dataset):
    lib = L.lib()
    V, m, pad, rows = c["V"], c["m"], c["pad"], c["rows"]
    tok, dY = C.emb_bwd_inputs(c, i, dataset)
    inp = inputs(dY=dY)
    tok_d = tok.cuda()
    tag = "embedding_bwd %s %s" % (C.emb_bwd_id(c), dataset)

    def run():
        fr = framed(dict(dtable=(V, m)))
        sc = framed(dict(scratch=(3 * V + 1 + rows,)), torch.int32)
        L.check(lib.sat_embedding_bwd(L.ptr(inp["dY"]), L.ptr(tok_d), dev(fr, "dtable", L), rows, V, m, pad, dev(sc, "scratch", L), L.stream_ptr()),
                "sat_embedding_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag); frames_intact(sc, tag)
        return dict(dtable=fr["dtable"][1])
    dtable = twice(run, tag)["dtable"]
    inputs_intact(inp, tag)
    assert R.canaries(dtable) == 0, tag + ": dtable is not fully overwritten"
    if dataset == "int":
        exact(dtable, R.embedding_bwd(dY, tok, V, pad), tag)
    else:
        want = R.embedding_bwd_chain_f32(dY, tok, V, pad)
        diff = bits(dtable) != bits(want)
        # +0 and -0: a row that sums to zero is as good either way
        assert not bool((diff & (dtable.cpu() != want)).any()), "%s: %d element(s) differ from the fp32 chain in increasing row order" % (tag, int(diff.sum()))
        close(dtable, R.embedding_bwd(dY, tok, V, pad), tag, "sat_embedding_bwd")


@pytest.mark.parametrize("i,c", _ids(C.EMB_FWD_CASES, C.emb_fwd_id))
def test_embedding_forward(L, i, c):
    """ids V and V + 3 address memory past the table: its frame is NaN and 4 m floats wide, so the read a kernel without the range check
    would make stays inside the test's own allocation and shows as NaN in the output"""
    lib = L.lib()
    V, m, mx = C.EMB_FWD_V, c["m"], c["max_norm"]
    table, tok = C.emb_fwd_inputs(c, i)
    rows = tok.numel()
    guard = max(R.GUARD, -(-4 * m // 4) * 4)
    assert guard >= (max(tok.tolist()) + 1 - V) * m
    tok_d = tok.cuda()
    tag = "embedding_fwd " + C.emb_fwd_id(c)

    def run():
        tw, tab = R.nan_framed(table, 0, guard)
        fr = framed(dict(out=(rows, m)))
        fl = framed(dict(flags=(V,) if mx > 0 else None), torch.int32)
        L.check(lib.sat_embedding_fwd(L.ptr(tab), L.ptr(tok_d), dev(fr, "out", L), rows, V, m, mx, dev(fl, "flags", L), L.stream_ptr()), "sat_embedding_fwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag); frames_intact(fl, tag)
        R.nan_frame_intact(tw, guard, tag + " table")
        return dict(out=fr["out"][1], table=tab)
    got = twice(run, tag)
    out, after = got["out"].cpu(), got["table"].cpu()
    assert not bool(torch.isnan(out).any()), tag + ": NaN in the gathered rows (a read outside the table)"
    want_out, want_table = R.embedding_fwd(table, tok, mx)
    ok = R.valid_tokens(tok, V)
    assert torch.equal(bits(out[ok]), bits(after[tok.long()[ok]])), tag + ": a gathered row is not the table's row"
    assert not bool(out[~ok].any()), tag + ": an id outside [0, V) does not give a zero row"
    rescaled = [v for v in C.EMB_FWD_BIG if v in tok.tolist()] if mx > 0 else []
    alone = [v for v in range(V) if v not in rescaled]
    assert torch.equal(bits(after[alone]), bits(table[alone])), tag + ": a row below max_norm, or one no token uses, changed"
    close(after, want_table, tag + " table", "sat_embedding_fwd")
    close(out, want_out, tag + " out", "sat_embedding_fwd")
    if rescaled:
        assert bool((after[rescaled].double().norm(dim=1) - mx).abs().max() < 1e-5), tag + ": a rescaled row does not have the norm max_norm"


# ------------------------------------------------------------------ sat_lstm_cell_fwd / sat_lstm_cell_bwd
def _lstm_forward(L, c, d, tag):
    lib = L.lib()
    N, n, inp = c["N"], c["n"], c["inp"]
    a = inputs(x=d["x"], h=d["h"], c=d["c"], w_ih=d["w_ih"], w_hh=d["w_hh"], b_ih=d["b_ih"], b_hh=d["b_hh"])

    def run():
        fr = framed(dict(gates=(N, 4 * n), h_new=(N, n), c_new=(N, n), bias=(4 * n,)))
        L.check(lib.sat_lstm_cell_fwd(L.ptr(a["x"]), inp, L.ptr(a["h"]), L.ptr(a["c"]), L.ptr(a["w_ih"]), L.ptr(a["w_hh"]), L.ptr(a["b_ih"]), L.ptr(a["b_hh"]),
                                      dev(fr, "gates", L), dev(fr, "h_new", L), dev(fr, "c_new", L), dev(fr, "bias", L), N, n, L.stream_ptr()), "sat_lstm_cell_fwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return {k: fr[k][1] for k in ("gates", "h_new", "c_new")}
    out = twice(run, tag)
    inputs_intact(a, tag)
    return a, out


def _lstm_backward(L, c, d, a, fwd, tag):
    lib = L.lib()
    N, n, inp = c["N"], c["n"], c["inp"]
    b = inputs(c_new=fwd["c_new"].cpu(), gates=fwd["gates"].cpu(), dh=d["dh"], dc=d["dc"])

    def run():
        fr = framed(dict(dx=(N, inp), dh_prev=(N, n), dc_prev=(N, n), dw_ih=(4 * n, inp), dw_hh=(4 * n, n), db_ih=(4 * n,), db_hh=(4 * n,), dgates=(N, 4 * n),
                         scratch=(-(-N // 256) * 4 * n,)))
        L.check(lib.sat_lstm_cell_bwd(L.ptr(a["x"]), inp, L.ptr(a["h"]), L.ptr(a["c"]), L.ptr(b["c_new"]), L.ptr(b["gates"]), L.ptr(b["dh"]), L.ptr(b["dc"]),
                                      L.ptr(a["w_ih"]), L.ptr(a["w_hh"]), *[dev(fr, k, L) for k in ("dx", "dh_prev", "dc_prev", "dw_ih", "dw_hh", "db_ih", "db_hh",
                                                                                                   "dgates", "scratch")], N, n, L.stream_ptr()), "sat_lstm_cell_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return {k: v for k, v in views(fr).items() if k != "scratch"}
    out = twice(run, tag)
    inputs_intact(a, tag); inputs_intact(b, tag)
    return out


LSTM = _ids(C.LSTM_CASES, C.lstm_id)


@pytest.mark.parametrize("i,c", [p for p in LSTM if p.values[1]["variant"] != "tiny"])
def test_lstm_cell(L, i, c):
    d = C.lstm_inputs(c, i)
    n, sat = c["n"], c["variant"] == "saturating"
    tag, entry = "lstm_cell " + C.lstm_id(c), "sat_lstm_cell (%s)" % c["variant"]
    rf = R.lstm_cell_fwd(d["x"], d["h"], d["c"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])
    a, fwd = _lstm_forward(L, c, d, tag)
    for k in ("gates", "h_new", "c_new"):
        assert bool(torch.isfinite(fwd[k]).all()), "%s: %s is not finite" % (tag, k)
        close(fwd[k], rf[k], "%s %s" % (tag, k), entry)
    assert float(fwd["h_new"].abs().max()) <= 1.0
    bwd = _lstm_backward(L, c, d, a, fwd, tag)
    rb = R.lstm_cell_bwd(d["x"], d["h"], d["c"], d["w_ih"], d["w_hh"], rf, d["dh"], d["dc"])
    for k in ("dgates", "dx", "dh_prev", "dc_prev", "dw_ih", "dw_hh"):
        assert bool(torch.isfinite(bwd[k]).all()), "%s: %s is not finite" % (tag, k)
        close(bwd[k], rb[k], "%s %s" % (tag, k), entry)
    close(bwd["db_ih"], rb["db"], tag + " db_ih", entry)
    assert torch.equal(bits(bwd["db_hh"]), bits(bwd["db_ih"])), tag + ": db_hh is not db_ih"
    if sat:
        g, dg = fwd["gates"].cpu(), bwd["dgates"].cpu()
        flat = torch.ones_like(g, dtype=torch.bool)
        flat[:, :2 * n] = (g[:, :2 * n] == 0) | (g[:, :2 * n] == 1)
        flat[:, 2 * n:3 * n] = g[:, 2 * n:3 * n].abs() == 1
        flat[:, 3 * n:] = (g[:, 3 * n:] == 0) | (g[:, 3 * n:] == 1)
        for q, name in enumerate("ifgo"):
            assert int(flat[:, q * n:(q + 1) * n].sum()) >= 5, "%s: gate %s is saturated to its limit in %d places only" % (tag, name, int(flat[:, q * n:(q + 1) * n].sum()))
        assert bool((g[:, :2 * n] == 0).any()) and bool((g[:, :2 * n] == 1).any())
        assert not bool(dg[flat].any()), "%s: %d gradient(s) of a saturated gate are not exactly zero" % (tag, int((dg[flat] != 0).sum()))


@pytest.mark.parametrize("i,c", [p for p in LSTM if p.values[1]["variant"] == "tiny"])
def test_lstm_cell_tiny_preactivations(L, i, c):
    d = C.lstm_inputs(c, i)
    tag = "lstm_cell " + C.lstm_id(c)
    rf = R.lstm_cell_fwd(d["x"], d["h"], d["c"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])
    _, fwd = _lstm_forward(L, c, d, tag)
    cell = nn.LSTMCell(c["inp"], c["n"])
    with torch.no_grad():
        for p, k in ((cell.weight_ih, "w_ih"), (cell.weight_hh, "w_hh"), (cell.bias_ih, "b_ih"), (cell.bias_hh, "b_hh")):
            p.copy_(d[k])
        h32, _ = cell(d["x"], (d["h"], d["c"]))
    e_cpu = float((h32.double() - rf["h_new"]).abs().max())
    e_gpu = float((fwd["h_new"].double().cpu() - rf["h_new"]).abs().max())
    bound = 4 * e_cpu + 4e-7
    WORST["sat_lstm_cell (tiny) |h - f64| / (4 e_cpu + 4e-7)"] = e_gpu / bound
    print("%s: max|h| = %.3e, e_gpu = %.3e, e_cpu(fp32 nn.LSTMCell) = %.3e, e_gpu / bound = %.3f" % (tag, float(rf["h_new"].abs().max()), e_gpu, e_cpu, e_gpu / bound))
    assert e_gpu <= bound, "%s: |h_new - float64| = %.3e > 4 * %.3e + 4e-7" % (tag, e_gpu, e_cpu)
    close(fwd["c_new"], rf["c_new"], tag + " c_new", "sat_lstm_cell (tiny)")


# ------------------------------------------------------------------ dropout masks
def mask_of(stream, count, p):
    from sat_amd.decoder import dropout_scale_reference
    return torch.from_numpy(dropout_scale_reference(SEED, stream, np.arange(count, dtype=np.uint64), p))


def kept_fraction_ok(mask, p, what):
    n = mask.numel()
    kept = float((mask != 0).sum()) / n
    sd = math.sqrt(p * (1 - p) / n)
    print("%s: kept %.4f of %d (1 - p = %.2f, 5 sd = %.4f)" % (what, kept, n, 1 - p, 5 * sd))
    assert abs(kept - (1 - p)) <= 5 * sd, "%s: kept fraction %.4f is not 1 - p = %.2f within 5 standard deviations (%.4f)" % (what, kept, 1 - p, 5 * sd)


# ------------------------------------------------------------------ sat_deep_output_fwd / sat_deep_output_bwd
# the integer data set pins db_out: it runs where the case asks for db_out
DEEP = [pytest.param(i, c, ds, id="%s-%s" % (C.deep_id(c), ds)) for i, c in enumerate(C.DEEP_CASES) for ds in ("real", "int") if ds == "real" or c["db"]]


@pytest.mark.parametrize("i,c,dataset", DEEP)
def test_deep_output(L, i, c, dataset):
    lib = L.lib()
    N, m, n, D, V, deep, p = c["N"], c["m"], c["n"], c["D"], c["V"], c["deep"], c["p"]
    d = C.deep_inputs(c, i, dataset)
    tag, entry = "deep_output %s %s" % (C.deep_id(c), dataset), "sat_deep_output (%s)" % ("deep" if deep else "shallow")
    mask = mask_of(2, N * m, p).reshape(N, m) if p > 0 else None
    a = inputs(prev=d["prev"] if deep else None, hidden=d["hidden"], context=d["context"] if deep else None, w_h=d["w_h"], w_c=d["w_c"] if deep else None,
               w_o=d["w_o"], b_o=d["b_o"], dlogits=d["dlogits"])

    def run_fwd():
        fr = framed(dict(u=(N, m), udrop=(N, m) if p > 0 else None, logits=(N, V)))
        L.check(lib.sat_deep_output_fwd(L.ptr(a["prev"]), L.ptr(a["hidden"]), L.ptr(a["context"]), L.ptr(a["w_h"]), L.ptr(a["w_c"]), L.ptr(a["w_o"]), L.ptr(a["b_o"]),
                                        p, SEED, dev(fr, "u", L), dev(fr, "udrop", L), dev(fr, "logits", L), N, m, n, D, V, L.stream_ptr()), "sat_deep_output_fwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return views(fr)
    fwd = twice(run_fwd, tag)
    rf = R.deep_output_fwd(d["prev"] if deep else None, d["hidden"], d["context"] if deep else None, d["w_h"], d["w_c"], d["w_o"], d["b_o"], mask)
    close(fwd["u"], rf["u"], tag + " u", entry)
    close(fwd["logits"], rf["logits"], tag + " logits", entry)
    if p > 0:
        u = fwd["u"].cpu()
        assert torch.equal(bits(fwd["udrop"]), bits(u * mask)), tag + ": udrop is not u times the mask (0 or 1 / (1 - p)), bit for bit"
        assert torch.equal(fwd["udrop"].cpu() == 0, mask == 0)
        if N * m >= 4096:
            kept_fraction_ok(fwd["udrop"].cpu(), p, tag)

    b = inputs(u=fwd["u"].cpu(), udrop=fwd["udrop"].cpu() if p > 0 else None)

    def run_bwd():
        fr = framed(dict(d_prev=(N, m), d_hidden=(N, n), d_context=(N, D) if deep else None, dw_hidden=(m, n), dw_context=(m, D) if deep else None, dw_out=(V, m),
                         db_out=(V,) if c["db"] else None, scratch=(-(-N // 256) * V,)))
        L.check(lib.sat_deep_output_bwd(L.ptr(a["dlogits"]), L.ptr(a["hidden"]), L.ptr(a["context"]), L.ptr(b["u"]), L.ptr(b["udrop"]), L.ptr(a["w_h"]), L.ptr(a["w_c"]),
                                        L.ptr(a["w_o"]), p, SEED, *[dev(fr, k, L) for k in ("d_prev", "d_hidden", "d_context", "dw_hidden", "dw_context", "dw_out",
                                                                                             "db_out", "scratch")], N, m, n, D, V, L.stream_ptr()), "sat_deep_output_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        if not c["db"]:
            R.all_canary(fr["scratch"][1], tag + " column-sum scratch without db_out")
        return {k: v for k, v in views(fr).items() if k != "scratch"}
    bwd = twice(run_bwd, tag)
    inputs_intact(a, tag); inputs_intact(b, tag)
    rb = R.deep_output_bwd(d["dlogits"], d["hidden"], d["context"] if deep else None, d["w_h"], d["w_c"], d["w_o"], rf, mask)
    for k, r in (("d_prev", "du"), ("d_hidden", "d_hidden"), ("dw_hidden", "dw_hidden"), ("dw_out", "dw_out")) + ((("d_context", "d_context"), ("dw_context", "dw_context")) if deep else ()):
        close(bwd[k], rb[r], "%s %s" % (tag, k), entry)
    if c["db"]:
        if dataset == "int":
            exact(bwd["db_out"], rb["db_out"], tag + " db_out")
        else:
            close(bwd["db_out"], rb["db_out"], tag + " db_out", entry)
    if p > 0 and not deep:          # the shallow form's d_prev_embed is the masked gradient itself: the forward's zero pattern
        assert torch.equal(rb["du"] == 0, mask == 0)
        assert torch.equal(bwd["d_prev"].cpu() == 0, rb["du"] == 0), tag + ": the backward's mask is not the forward's"


# ------------------------------------------------------------------ sat_init_lstm_fwd / sat_init_lstm_bwd
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.INIT_CASES, C.init_id))
def test_init_lstm(L, i, c, dataset):
    lib = L.lib()
    N, Lc, D, m, n2, p = c["N"], c["L"], c["D"], c["m"], c["n2"], c["p"]
    d = C.init_inputs(c, i, dataset)
    tag, entry = "init_lstm %s %s" % (C.init_id(c), dataset), "sat_init_lstm"
    mask = mask_of(0, N * D, p).reshape(N, D) if p > 0 else None
    a = inputs(ann=d["ann"], w_f=d["w_f"], b_f=d["b_f"], w_i=d["w_i"], b_i=d["b_i"], dinit=d["dinit"])

    def forward(drop):
        def run():
            fr = framed(dict(mean=(N, D), f=(N, m), init=(N, n2)))
            L.check(lib.sat_init_lstm_fwd(L.ptr(a["ann"]), L.ptr(a["w_f"]), L.ptr(a["b_f"]), L.ptr(a["w_i"]), L.ptr(a["b_i"]), drop, SEED, dev(fr, "mean", L),
                                          dev(fr, "f", L), dev(fr, "init", L), N, Lc, D, m, n2, L.stream_ptr()), "sat_init_lstm_fwd")
            torch.cuda.synchronize()
            frames_intact(fr, tag)
            return views(fr)
        return run
    fwd = twice(forward(p), tag)
    rf = R.init_lstm_fwd(d["ann"], d["w_f"], d["b_f"], d["w_i"], d["b_i"], mask)
    for k in ("mean", "f", "init"):
        close(fwd[k], rf[k], "%s %s" % (tag, k), entry)
    if p > 0:
        plain = forward(0.0)()["mean"].cpu()
        assert torch.equal(bits(fwd["mean"]), bits(plain * mask)), tag + ": the dropped mean is not the mean times the mask (0 or 1 / (1 - p)), bit for bit"
        if N * D >= 4096:
            kept_fraction_ok(fwd["mean"].cpu(), p, tag)

    b = inputs(mean=fwd["mean"].cpu(), f=fwd["f"].cpu())

    def run_bwd():
        fr = framed(dict(dw_f=(m, D), db_f=(m,), dw_i=(n2, m), db_i=(n2,), dann=(N, Lc, D), df=(N, m), dmean=(N, D), scratch=(-(-N // 256) * max(n2, m),)))
        L.check(lib.sat_init_lstm_bwd(L.ptr(a["dinit"]), L.ptr(b["mean"]), L.ptr(b["f"]), L.ptr(a["w_f"]), L.ptr(a["w_i"]), p, SEED,
                                      *[dev(fr, k, L) for k in ("dw_f", "db_f", "dw_i", "db_i", "dann", "df", "dmean", "scratch")], N, Lc, D, m, n2, L.stream_ptr()),
                "sat_init_lstm_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return {k: v for k, v in views(fr).items() if k != "scratch"}
    bwd = twice(run_bwd, tag)
    inputs_intact(a, tag); inputs_intact(b, tag)
    rb = R.init_lstm_bwd(d["dinit"], d["w_f"], d["w_i"], rf, Lc, mask)
    for k in ("dw_f", "db_f", "dw_i", "db_i", "dann", "df", "dmean"):
        close(bwd[k], rb[k], "%s %s" % (tag, k), entry)
    if dataset == "int":
        for k in ("db_i", "df", "db_f") + (("dmean",) if p == 0 else ()) + (("dann",) if p == 0 and Lc & (Lc - 1) == 0 else ()):
            exact(bwd[k], rb[k], "%s %s" % (tag, k))
    if p > 0:          # zero where the forward's mask is zero and nowhere else (integers: also where the gradient itself cancels to 0)
        assert dataset == "int" or torch.equal(rb["dmean"] == 0, mask == 0)
        assert torch.equal(bwd["dmean"].cpu() == 0, rb["dmean"] == 0), tag + ": the backward's mask is not the forward's"


# ------------------------------------------------------------------ sat_doubly_stochastic_fwd / sat_doubly_stochastic_bwd
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.DS_CASES, C.ds_id))
def test_doubly_stochastic(L, i, c, dataset):
    lib = L.lib()
    N, Lc, T1, gamma, gs = c["N"], c["L"], c["T1"], c["gamma"], c["gscale"]
    alphas = C.ds_inputs(c, i, dataset)
    tag, entry = "doubly_stochastic %s %s" % (C.ds_id(c), dataset), "sat_doubly_stochastic"
    nb = -(-N * Lc // 256)
    a = inputs(alphas=alphas, gscale=torch.tensor([gs]) if gs is not None else None)

    def run():
        fr = framed(dict(asum=(N, Lc), part=(nb,), out=(1,)))
        L.check(lib.sat_doubly_stochastic_fwd(L.ptr(a["alphas"]), N, T1, Lc, gamma, dev(fr, "asum", L), dev(fr, "part", L), dev(fr, "out", L), L.stream_ptr()),
                "sat_doubly_stochastic_fwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        assert R.canaries(fr["part"][1]) == 0
        return dict(asum=fr["asum"][1], out=fr["out"][1])
    fwd = twice(run, tag)
    asum, out = R.doubly_stochastic_fwd(alphas, gamma)
    if dataset == "int":
        exact(fwd["asum"], asum, tag + " asum")
        total = float(((1 - asum) ** 2).sum())          # an integer below 2^53; every block partial an integer below 2^24
        want = np.float32(gamma) * np.float32(total / (N * Lc))
        assert float(fwd["out"].cpu()[0]) == float(want), "%s out: %r is not gamma * mean = %r" % (tag, float(fwd["out"].cpu()[0]), float(want))
    else:
        close(fwd["asum"], asum, tag + " asum", entry)
        close(fwd["out"], out.reshape(1), tag + " out", entry)

    b = inputs(asum=fwd["asum"].cpu())

    def run_bwd():
        fr = framed(dict(dalphas=(N, T1, Lc)))
        L.check(lib.sat_doubly_stochastic_bwd(L.ptr(b["asum"]), L.ptr(a["gscale"]), N, T1, Lc, gamma, dev(fr, "dalphas", L), L.stream_ptr()), "sat_doubly_stochastic_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return views(fr)
    dal = twice(run_bwd, tag)["dalphas"]
    inputs_intact(a, tag); inputs_intact(b, tag)
    ref = R.doubly_stochastic_bwd(fwd["asum"].cpu(), gamma, None if gs is None else float(np.float32(gs)), T1)
    close(dal, ref, tag + " dalphas", entry)
    err, top = float((dal.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print("%s dalphas: max|d| / max|ref| = %.3e" % (tag, err / top))
    assert err <= 8 * 2.0 ** -24 * top, "%s dalphas: max|d| = %.3e > 8 u max|ref| = %.3e" % (tag, err, 8 * 2.0 ** -24 * top)


# ------------------------------------------------------------------ sat_sigmoid_bwd
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.SIGMOID_CASES, lambda c: "n%d" % c["n"]))
def test_sigmoid_backward(L, i, c, dataset):
    lib = L.lib()
    n = c["n"]
    dy, y = C.sigmoid_inputs(c, i, dataset)
    a = inputs(dy=dy, y=y)
    tag = "sigmoid_bwd n%d %s" % (n, dataset)

    def run():
        fr = framed(dict(dpre=(n,)))
        L.check(lib.sat_sigmoid_bwd(L.ptr(a["dy"]), L.ptr(a["y"]), dev(fr, "dpre", L), n, L.stream_ptr()), "sat_sigmoid_bwd")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return views(fr)
    dpre = twice(run, tag)["dpre"]
    inputs_intact(a, tag)
    if dataset == "int":
        exact(dpre, R.sigmoid_bwd(dy, y), tag)
    else:
        close(dpre, R.sigmoid_bwd(dy, y), tag, "sat_sigmoid_bwd")


# ------------------------------------------------------------------ sat_topk
@pytest.mark.parametrize("i,c", [pytest.param(i, c, id=C.topk_id(i, c)) for i, c in enumerate(C.TOPK_CASES)])
def test_topk(L, i, c):
    lib = L.lib()
    n, k = c["n"], c["k"]
    x = C.topk_inputs(c, i)
    a = inputs(x=x)
    tag = "topk " + C.topk_id(i, c)

    def run():
        fr = framed(dict(work=(n,), values=(k,)))
        ix = framed(dict(indices=(k,)), torch.int32)
        L.check(lib.sat_topk(L.ptr(a["x"]), dev(fr, "work", L), n, k, dev(fr, "values", L), dev(ix, "indices", L), L.stream_ptr()), "sat_topk")
        torch.cuda.synchronize()
        frames_intact(fr, tag); frames_intact(ix, tag)
        return dict(values=fr["values"][1], indices=ix["indices"][1])
    got = twice(run, tag)
    inputs_intact(a, tag)
    assert torch.equal(bits(a["x"]), bits(x)), tag + ": x was written"
    vals, idx = R.ref_topk(x, k)
    gi = got["indices"].cpu().long()
    assert len(set(gi.tolist())) == k, "%s: an index is returned twice: %s" % (tag, gi.tolist()[:16])
    assert gi.tolist() == idx.tolist(), "%s: indices %s, the stable descending sort gives %s" % (tag, gi.tolist()[:16], idx.tolist()[:16])
    assert torch.equal(bits(got["values"]), bits(x[gi])), tag + ": a value is not x at its index"


# ------------------------------------------------------------------ sat_beam_scores
@pytest.mark.parametrize("i,c", _ids(C.BEAM_CASES, C.beam_id))
def test_beam_scores(L, i, c):
    import test_gpu_search_history as H          # the bound and its magnitude are derived and restated there
    lib = L.lib()
    V, T = c["V"], c["T"]
    x, parent = C.beam_inputs(c, i)
    rows = x.shape[0]
    masked = C.beam_masked(c)
    a = inputs(x=x, parent=parent)
    masked_d = torch.tensor(masked, dtype=torch.int32, device="cuda")
    tag = "beam_scores " + C.beam_id(c)

    def run():
        fr = framed(dict(scores=(rows, V)))
        L.check(lib.sat_beam_scores(L.ptr(a["x"]), rows, V, T, L.ptr(masked_d), len(masked), L.ptr(a["parent"]), dev(fr, "scores", L), L.stream_ptr()), "sat_beam_scores")
        torch.cuda.synchronize()
        frames_intact(fr, tag)
        return views(fr)
    got = twice(run, tag)["scores"].double().cpu()
    inputs_intact(a, tag)
    want = R.beam_scores(x, T, masked, parent)
    assert not bool(torch.isnan(got).any()), "%s: NaN in rows %s" % (tag, torch.nonzero(torch.isnan(got).any(1)).reshape(-1).tolist())
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)), tag + ": the -inf positions differ"
    bound_u = (math.ceil(V / 256) + 32) * 2.0 ** -24
    worst = 0.0
    for r in range(rows):
        live = torch.isfinite(x[r])
        par = parent[r:r + 1].numpy() if parent is not None else None
        s, mag = H._restate(x[r, live][None].numpy(), T, [], par, np.zeros((1, 1), np.int64), [0], (0, 0, 1.0), 0, 0)
        assert np.allclose(s[0], R.beam_scores(x[r:r + 1], T, [], parent[r:r + 1] if parent is not None else None)[0, live].numpy(), rtol=0, atol=1e-9)
        fin = torch.isfinite(want[r])
        ratio = float((got[r, fin] - want[r, fin]).abs().max()) / (bound_u * float(mag[0])) if bool(fin.any()) else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s row %d: error / bound = %.3f (bound %.3e)" % (tag, r, ratio, bound_u * float(mag[0]))
    WORST["sat_beam_scores error / bound"] = max(WORST.get("sat_beam_scores error / bound", 0.0), worst)
    print("%s: worst error / bound %.3f" % (tag, worst))
