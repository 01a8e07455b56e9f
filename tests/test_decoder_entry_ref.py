"""CPU: the float64 restatements of tests/decoder_entry_ref.py and the inputs of tests/decoder_entry_cases.py, before
test_gpu_decoder_entry_points.py compares the kernels with them.

1. Each restatement agrees with torch's own module in float64 (nn.LSTMCell, nn.Embedding with max_norm and padding_idx through
   autograd, torch.log_softmax) and with oracle/sat_oracle.py (InitLSTM with its raw reshape, DeepOutput deep and shallow).
2. The tables reach what they claim: both column-sum paths, every occurrence count of the embedding gradient, both of its paths.
3. Sensitivity.  A comparison proves something only if the reference itself would notice the mistake.  On every case's inputs the
   reference is evaluated again without the last row, the last column (of the output, or of a product's inner dimension), the last
   token occurrence or the last time step, the result padded back with zeros -- what a kernel that skips the element leaves -- and
   every compared output that depends on the element must move by at least 100 bounds of the GPU comparison,
   1e-4 max(1, max|ref|); the integer data sets, compared bit for bit, by at least 1 (by an fp32 ulp of the mean for `out` of the
   doubly stochastic term).  Exempt by the formula: `out` of the doubly stochastic term, a mean over N L elements, of one real element.
4. ref_topk returns every index once, and a simulation of the knock-out rule csrc/decoder_kernels.h had before this file existed
   (winners overwritten with -inf, the scan taking v == best && i < best_i from best = -inf) shows the repeated index that rule gives
   as soon as fewer than k entries above -inf are left; the rule it has now (winners marked apart from -inf) is ref_topk."""
import numpy as np
import pytest
import torch
from torch import nn

import decoder_entry_cases as C
import decoder_entry_ref as R

TOL = 1e-4          # the bound of test_gpu_decoder_entry_points.py
D64 = torch.float64


def _ids(cases, fn):
    return [pytest.param(i, c, id=fn(c)) for i, c in enumerate(cases)]


def _pad(t, shape):
    out = torch.zeros(shape, dtype=t.dtype)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out


def _noticed(full, cut, what, exact=False):
    """`cut` (smaller shapes are padded with zeros) differs from `full` by 100 bounds, or by 1 for the integer data sets"""
    full = full.reshape(1) if full.dim() == 0 else full
    cut = _pad(cut.reshape(1) if cut.dim() == 0 else cut, full.shape)
    moved = float((full - cut).abs().max())
    bound = 1.0 if exact else 100 * TOL * max(1.0, float(full.abs().max()))
    assert moved >= bound, "%s: the reference moves by %.3g < %.3g" % (what, moved, bound)


# ------------------------------------------------------------------ 1. the restatements against torch and the oracle
def test_lstm_cell_restatement_is_nn_lstmcell():
    g = torch.Generator().manual_seed(1)
    N, n, inp = 6, 5, 7
    cell = nn.LSTMCell(inp, n).double()
    x, h, c = (torch.randn(N, k, generator=g, dtype=D64).requires_grad_() for k in (inp, n, n))
    dh, dc = torch.randn(N, n, generator=g, dtype=D64), torch.randn(N, n, generator=g, dtype=D64)
    hn, cn = cell(x, (h, c))
    ((hn * dh).sum() + (cn * dc).sum()).backward()
    w = [p.detach() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)]
    f = R.lstm_cell_fwd(x, h, c, *w)
    assert torch.allclose(f["h_new"], hn.detach(), rtol=0, atol=1e-13) and torch.allclose(f["c_new"], cn.detach(), rtol=0, atol=1e-13)
    b = R.lstm_cell_bwd(x, h, c, w[0], w[1], f, dh, dc)
    for got, want in ((b["dx"], x.grad), (b["dh_prev"], h.grad), (b["dc_prev"], c.grad), (b["dw_ih"], cell.weight_ih.grad),
                      (b["dw_hh"], cell.weight_hh.grad), (b["db"], cell.bias_ih.grad), (b["db"], cell.bias_hh.grad)):
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # without dc_new: the gradient through h_new alone
    for p in (x, h, c, *cell.parameters()):
        p.grad = None
    hn, _ = cell(x, (h, c))
    (hn * dh).sum().backward()
    b = R.lstm_cell_bwd(x, h, c, w[0], w[1], f, dh, None)
    assert torch.allclose(b["dx"], x.grad, rtol=0, atol=1e-12) and torch.allclose(b["dc_prev"], c.grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("pad", [0, -1])
def test_embedding_restatements_are_nn_embedding(pad):
    g = torch.Generator().manual_seed(2)
    V, m = 9, 4
    table = torch.randn(V, m, generator=g, dtype=D64) * torch.tensor([0.1, 3, 0.1, 3, 1, 1, 0.1, 3, 1], dtype=D64)[:, None]
    tok = torch.tensor([1, 2, 1, 0, 8, 1, 3, 0])
    emb = nn.Embedding(V, m, padding_idx=pad if pad >= 0 else None, max_norm=1.5).double()
    with torch.no_grad():
        emb.weight.copy_(table)
    out = emb(tok)
    want_out, want_table = R.embedding_fwd(table, tok.int(), 1.5)
    assert torch.allclose(out.detach(), want_out, rtol=0, atol=1e-13) and torch.allclose(emb.weight.detach(), want_table, rtol=0, atol=1e-13)
    assert torch.equal(want_table[[2, 4, 5, 6, 7]], table[[2, 4, 5, 6, 7]])          # below max_norm, or not used: untouched
    dY = torch.randn(len(tok), m, generator=g, dtype=D64)
    (out * dY).sum().backward()
    assert torch.allclose(R.embedding_bwd(dY, tok.int(), V, pad), emb.weight.grad, rtol=0, atol=1e-13)
    # ids outside [0, V): zero rows forward, skipped backward (torch refuses them)
    tok2 = torch.tensor([1, -1, V, V + 3, 8], dtype=torch.int32)
    o2, _ = R.embedding_fwd(table, tok2, 0.0)
    assert torch.equal(o2[[0, 4]], table[[1, 8]]) and not o2[1:4].any()
    g2 = R.embedding_bwd(dY[:5], tok2, V, -1)
    assert torch.equal(g2[1], dY[0]) and torch.equal(g2[8], dY[4]) and float(g2.abs().sum()) == float(dY[[0, 4]].abs().sum())
    # the fp32 chain is the same sum
    chain = R.embedding_bwd_chain_f32(dY.float(), tok.int(), V, pad)
    assert torch.allclose(chain.double(), R.embedding_bwd(dY.float(), tok.int(), V, pad), rtol=0, atol=1e-5)


@pytest.mark.parametrize("deep", [True, False])
def test_deep_output_restatement_is_the_oracle(deep):
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(3)
    N, m, n, D, V = 5, 6, 4, 7, 11
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    sd = {"output.hidden.weight": r(m, n).requires_grad_(), "output.context.weight": r(m, D).requires_grad_(),
          "output.output.weight": r(V, m).requires_grad_(), "output.output.bias": r(V).requires_grad_()}
    y, h, z = r(N, m).requires_grad_(), r(N, n).requires_grad_(), r(N, D).requires_grad_()
    mask = (torch.rand(N, m, generator=g) > 0.4).double() / 0.6
    dl = r(N, V)
    logits = O.deep_output(sd, y, h, z, deep=deep, x_mask=mask)
    (logits * dl).sum().backward()
    w = [sd[k].detach() for k in ("output.hidden.weight", "output.context.weight", "output.output.weight", "output.output.bias")]
    f = R.deep_output_fwd(y if deep else None, h, z if deep else None, w[0], w[1], w[2], w[3], mask)
    assert torch.allclose(f["logits"], logits.detach(), rtol=0, atol=1e-12)
    b = R.deep_output_bwd(dl, h, z if deep else None, w[0], w[1], w[2], f, mask)
    pairs = [(b["d_hidden"], h.grad), (b["dw_hidden"], sd["output.hidden.weight"].grad), (b["dw_out"], sd["output.output.weight"].grad),
             (b["db_out"], sd["output.output.bias"].grad)]
    if deep:
        pairs += [(b["du"], y.grad), (b["d_context"], z.grad), (b["dw_context"], sd["output.context.weight"].grad)]
    for got, want in pairs:
        assert torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("layers", [1, 2])
def test_init_lstm_restatement_is_the_oracle_with_its_raw_reshape(layers):
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(4)
    N, Hh, Ww, D, m, n = 5, 2, 3, 7, 4, 3
    L, n2 = Hh * Ww, 2 * layers * n
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    sd = {"init_lstm.factorize.weight": r(m, D).requires_grad_(), "init_lstm.factorize.bias": r(m).requires_grad_(),
          "init_lstm.init.weight": r(n2, m).requires_grad_(), "init_lstm.init.bias": r(n2).requires_grad_()}
    ann = r(N, D, Hh, Ww).requires_grad_()
    mask = (torch.rand(N, D, generator=g) > 0.3).double() / 0.7
    h0, c0 = O.init_state(sd, ann, layers, n, mean_mask=mask)
    dh, dc = r(layers, N, n), r(layers, N, n)
    ((h0 * dh).sum() + (c0 * dc).sum()).backward()
    w = [sd[k].detach() for k in ("init_lstm.factorize.weight", "init_lstm.factorize.bias", "init_lstm.init.weight", "init_lstm.init.bias")]
    a = ann.detach().reshape(N, D, L).permute(0, 2, 1)
    f = R.init_lstm_fwd(a, *w, mask)
    # `init` (N, n2) row-major is the (2 layers, N, n) buffer: h0 the first layers N n floats, c0 the rest
    flat = f["init"].reshape(-1)
    assert torch.allclose(flat[:layers * N * n], h0.detach().reshape(-1), rtol=0, atol=1e-12)
    assert torch.allclose(flat[layers * N * n:], c0.detach().reshape(-1), rtol=0, atol=1e-12)
    b = R.init_lstm_bwd(torch.cat([dh.reshape(-1), dc.reshape(-1)]).reshape(N, n2), w[0], w[2], f, L, mask)
    for got, want in ((b["dw_f"], sd["init_lstm.factorize.weight"].grad), (b["db_f"], sd["init_lstm.factorize.bias"].grad),
                      (b["dw_i"], sd["init_lstm.init.weight"].grad), (b["db_i"], sd["init_lstm.init.bias"].grad),
                      (b["dann"], ann.grad.reshape(N, D, L).permute(0, 2, 1))):
        assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_small_restatements_are_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 17, generator=g, dtype=D64) * 3
    x[1, 4] = -np.inf
    parent = torch.randn(3, generator=g, dtype=D64)
    s = R.beam_scores(x.float(), 0.7, [2, -1, 17, 30], parent)
    want = torch.log_softmax(x.float().double() / float(np.float32(0.7)), 1) + parent[:, None]
    keep = torch.ones(17, dtype=torch.bool); keep[2] = False
    assert torch.equal(s[:, keep], want[:, keep]) and bool(torch.isneginf(s[:, 2]).all()) and bool(torch.isneginf(s[1, 4]))
    assert bool(torch.isnan(torch.log_softmax(torch.full((1, 4), -np.inf, dtype=D64), 1)).all())          # what an all -inf row gives
    # doubly stochastic term and its gradient; sigmoid backward
    a = torch.rand(4, 3, 5, generator=g, dtype=D64).requires_grad_()
    out = 0.7 * ((1 - a.sum(1)) ** 2).mean()
    (out * 3.0).backward()
    asum, want = R.doubly_stochastic_fwd(a.detach(), 0.7)
    assert abs(float(out.detach()) - float(want)) < 1e-6          # gamma enters as the fp32 0.7 the kernel is given
    assert torch.allclose(R.doubly_stochastic_bwd(asum, 0.7, 3.0, 3), a.grad, rtol=0, atol=1e-7)
    p = torch.randn(9, generator=g, dtype=D64).requires_grad_()
    y = torch.sigmoid(p); dy = torch.randn(9, generator=g, dtype=D64)
    (y * dy).sum().backward()
    assert torch.allclose(R.sigmoid_bwd(dy, y.detach()), p.grad, rtol=0, atol=1e-14)
    assert torch.equal(R.colsum(x[:, :3]), x[:, :3].sum(0))


# ------------------------------------------------------------------ 2. the tables reach what they claim
def test_tables_reach_every_path():
    assert all(C.colsum_path(c) == c["path"] for c in C.COLSUM_CASES)
    for path, cols in (("vec", {4, 36, 512, 516}), ("scalar", {1, 23, 257, 36})):
        assert {c["cols"] for c in C.COLSUM_CASES if c["path"] == path} == cols
    assert {c["rows"] for c in C.COLSUM_CASES} == {1, 3, 4, 5, 255, 256, 257, 513}
    assert any(c["path"] == "vec" and c["ld"] > c["cols"] for c in C.COLSUM_CASES)
    assert any(c["path"] == "scalar" and c["ld"] == 37 for c in C.COLSUM_CASES) and any(c["off"] == 1 for c in C.COLSUM_CASES)
    counts, unused, skipped = set(), False, set()
    for c in C.EMB_BWD_CASES:
        tok = C.emb_bwd_tokens(c)
        occ = C.occurrences(tok, c["V"], c["pad"])
        counts |= set(occ.values())
        unused |= len(occ) < c["V"]
        skipped |= {"-1"} if bool((tok == -1).any()) else set()
        skipped |= {">=V"} if bool((tok >= c["V"]).any()) else set()
        skipped |= {"pad"} if c["pad"] >= 0 and bool((tok == c["pad"]).any()) else set()
        assert tok.numel() == c["rows"] and c["rows"] % 256 != 0
    assert {1, 2, 3, 1023, 1024, 1025, 1280, 2049 + 7} <= counts and unused and skipped == {"-1", ">=V", "pad"}
    assert max(v for v in counts if v <= C.EMB_LIST) == C.EMB_LIST and min(v for v in counts if v > C.EMB_LIST) == C.EMB_LIST + 1
    assert {c["V"] for c in C.EMB_BWD_CASES} == {1, 1024, 1025, 2049} and {c["m"] for c in C.EMB_BWD_CASES} >= {1, 255, 256, 257}
    assert {c["pad"] for c in C.EMB_BWD_CASES} == {0, -1}
    assert {c["m"] for c in C.EMB_FWD_CASES} == {1, 63, 64, 65, 300}
    assert {c["N"] * c["n"] for c in C.LSTM_CASES} >= {255, 256, 257} and {c["variant"] for c in C.LSTM_CASES} == {"real", "saturating", "tiny"}
    assert {(c["deep"], c["p"] > 0) for c in C.DEEP_CASES} == {(True, False), (True, True), (False, False), (False, True)}
    assert {c["V"] for c in C.DEEP_CASES} == {23, 24, 1003} and any(not c["db"] for c in C.DEEP_CASES) and any(c["N"] * c["m"] >= 4096 and c["p"] > 0 for c in C.DEEP_CASES)
    assert {c["N"] * c["L"] for c in C.DS_CASES} == {255, 256, 257, 70000} and {c["T1"] for c in C.DS_CASES} == {1, 9}
    assert {c["n"] for c in C.TOPK_CASES} >= {1, 63, 64, 65, 1023, 1024, 1025, 50000}
    assert {c["V"] for c in C.BEAM_CASES} == {1, 255, 256, 257, 10000}


def test_saturating_and_tiny_inputs_are_what_they_say():
    for i, c in enumerate(C.LSTM_CASES):
        d = C.lstm_inputs(c, i)
        pre = R.lstm_cell_fwd(d["x"], d["h"], d["c"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])["pre"]
        if c["variant"] == "saturating":
            for gate in pre.chunk(4, dim=1):          # each of i, f, g, o is driven past +-200 and into +-(40 .. 88)
                assert float(gate.max()) > 200 and float(gate.min()) < -200
                assert bool(((gate > 40) & (gate < 88)).any()) and bool(((gate < -40) & (gate > -88)).any())
            assert float(d["c"].abs().max()) > 28
        elif c["variant"] == "tiny":
            assert 1e-4 < float(pre.abs().max()) < 2e-3 and float(d["c"].abs().max()) < 1e-3
        else:
            assert 2 < float(pre.abs().max()) < 40


# ------------------------------------------------------------------ 3. sensitivity
@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.COLSUM_CASES, C.colsum_id))
def test_colsum_reference_notices_the_last_row_and_column(i, c, dataset):
    x = C.colsum_inputs(c, i, dataset)
    full = R.colsum(x)
    _noticed(full, R.colsum(x[:-1]), "last row", dataset == "int")
    _noticed(full, R.colsum(x[:, :-1]), "last column", dataset == "int")
    if dataset == "int":
        assert float(x.abs().max()) <= 8 and bool((x == x.round()).all())


@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", _ids(C.EMB_BWD_CASES, C.emb_bwd_id))
def test_embedding_gradient_reference_notices_the_last_occurrence(i, c, dataset):
    tok, dY = C.emb_bwd_inputs(c, i, dataset)
    full = R.embedding_bwd(dY, tok, c["V"], c["pad"])
    for t, _, _ in c["plan"]:
        cut = tok.clone()
        cut[int(torch.nonzero(tok == t)[-1])] = -1
        less = R.embedding_bwd(dY, cut, c["V"], c["pad"])
        assert torch.equal(less[torch.arange(c["V"]) != t], full[torch.arange(c["V"]) != t])
        _noticed(full, less, "last occurrence of token %d" % t, dataset == "int")
    _noticed(full, R.embedding_bwd(dY[:, :-1], tok, c["V"], c["pad"]), "last column", dataset == "int")
    if c["pad"] >= 0:
        assert not full[c["pad"]].any()


@pytest.mark.parametrize("i,c", _ids(C.EMB_FWD_CASES, C.emb_fwd_id))
def test_embedding_forward_inputs(i, c):
    table, tok = C.emb_fwd_inputs(c, i)
    norm = table.double().norm(dim=1)
    assert bool((norm[list(C.EMB_FWD_BIG)] > 2.9).all()) and bool((norm[list(C.EMB_FWD_SMALL)] < 0.51).all())
    out, after = R.embedding_fwd(table, tok, c["max_norm"])
    _noticed(out, out[:-1], "last token")
    _noticed(out, out[:, :-1], "last column")
    used_big = [v for v in C.EMB_FWD_BIG if v in tok.tolist()]
    changed = (after != table.double()).any(1)
    assert changed.tolist() == [c["max_norm"] > 0 and v in used_big for v in range(C.EMB_FWD_V)]
    assert int((tok == 2).sum()) == 3 and {-1, C.EMB_FWD_V, C.EMB_FWD_V + 3} <= set(tok.tolist())


@pytest.mark.parametrize("i,c", [p for p in _ids(C.LSTM_CASES, C.lstm_id) if p.values[1]["variant"] == "real"])
def test_lstm_reference_notices_every_last_element(i, c):
    d = C.lstm_inputs(c, i)
    N, n, inp = c["N"], c["n"], c["inp"]
    w = (d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])
    f = R.lstm_cell_fwd(d["x"], d["h"], d["c"], *w)
    b = R.lstm_cell_bwd(d["x"], d["h"], d["c"], w[0], w[1], f, d["dh"], d["dc"])
    f_in = R.lstm_cell_fwd(d["x"][:, :-1], d["h"], d["c"], w[0][:, :-1], w[1], w[2], w[3])
    f_hid = R.lstm_cell_fwd(d["x"], d["h"][:, :-1], d["c"], w[0], w[1][:, :-1], w[2], w[3])
    for k in ("gates", "h_new", "c_new"):
        _noticed(f[k], f[k][:-1], "%s without the last row" % k)
        _noticed(f[k], f_in[k], "%s without the last input column" % k)
        _noticed(f[k], f_hid[k], "%s without the last hidden unit in the recurrent product" % k)
        _noticed(f[k], f[k][:, :-1], "%s without its last column" % k)
    for k in ("dgates", "dx", "dh_prev", "dc_prev"):
        _noticed(b[k], b[k][:-1], "%s without the last row" % k)
    if N > 1:
        f1 = {k: v[:-1] for k, v in f.items()}
        b1 = R.lstm_cell_bwd(d["x"][:-1], d["h"][:-1], d["c"][:-1], w[0], w[1], f1, d["dh"][:-1], None if d["dc"] is None else d["dc"][:-1])
        for k in ("dw_ih", "dw_hh", "db"):
            _noticed(b[k], b1[k], "%s without the last row" % k)
    dg = b["dgates"][:, :-1].double()
    _noticed(b["dx"], dg @ d["w_ih"].double()[:-1], "dx without the last gate column")
    _noticed(b["dh_prev"], dg @ d["w_hh"].double()[:-1], "dh_prev without the last gate column")


@pytest.mark.parametrize("i,c", _ids(C.DEEP_CASES, C.deep_id))
def test_deep_output_reference_notices_every_last_element(i, c):
    d = C.deep_inputs(c, i)
    deep = c["deep"]
    args = lambda **o: {**dict(prev_embed=d["prev"] if deep else None, hidden=d["hidden"], context=d["context"] if deep else None, w_h=d["w_h"], w_c=d["w_c"],
                               w_o=d["w_o"], b_o=d["b_o"]), **o}
    f = R.deep_output_fwd(**args())
    _noticed(f["logits"], f["logits"][:-1], "logits without the last row")
    _noticed(f["logits"], f["logits"][:, :-1], "logits without the last word")
    ud = f["udrop"]
    _noticed(f["logits"], ud[:, :-1] @ d["w_o"].double()[:, :-1].t() + d["b_o"].double(), "logits without the last unit of m")
    _noticed(f["u"], R.deep_output_fwd(**args(hidden=d["hidden"][:, :-1], w_h=d["w_h"][:, :-1]))["u"], "u without the last unit of n")
    if deep:
        _noticed(f["u"], R.deep_output_fwd(**args(context=d["context"][:, :-1], w_c=d["w_c"][:, :-1]))["u"], "u without the last feature")
    for dataset in ("real", "int"):
        dl = C.deep_inputs(c, i, dataset)["dlogits"]
        b = R.deep_output_bwd(dl, d["hidden"], d["context"] if deep else None, d["w_h"], d["w_c"], d["w_o"], f)
        _noticed(b["db_out"], dl.double()[:-1].sum(0), "db_out without the last row (%s)" % dataset, dataset == "int")
        _noticed(b["db_out"], b["db_out"][:-1], "db_out without the last word (%s)" % dataset, dataset == "int")
    dlr = d["dlogits"]
    b = R.deep_output_bwd(dlr, d["hidden"], d["context"] if deep else None, d["w_h"], d["w_c"], d["w_o"], f)
    b1 = R.deep_output_bwd(dlr[:, :-1], d["hidden"], d["context"] if deep else None, d["w_h"], d["w_c"], d["w_o"][:-1], f)
    for k in ("du", "d_hidden"):
        _noticed(b[k], b1[k], "%s without the last word in the product" % k)
    fm = {k: v[:-1] for k, v in f.items()}
    bm = R.deep_output_bwd(dlr[:-1], d["hidden"][:-1], d["context"][:-1] if deep else None, d["w_h"], d["w_c"], d["w_o"], fm)
    for k in ("dw_out", "dw_hidden") + (("dw_context",) if deep else ()):
        _noticed(b[k], bm[k], "%s without the last row" % k)


@pytest.mark.parametrize("i,c", _ids(C.INIT_CASES, C.init_id))
def test_init_lstm_reference_notices_every_last_element(i, c):
    d = C.init_inputs(c, i)
    w = (d["w_f"], d["b_f"], d["w_i"], d["b_i"])
    f = R.init_lstm_fwd(d["ann"], *w)
    no_last = d["ann"].clone()
    no_last[:, -1] = 0          # a mean that skips the last location still divides by L
    cut = R.init_lstm_fwd(no_last, *w)
    for k in ("mean", "f", "init"):
        _noticed(f[k], f[k][:-1], "%s without the last row" % k)
        _noticed(f[k], cut[k], "%s without the last location" % k)
    _noticed(f["f"], R.init_lstm_fwd(d["ann"][:, :, :-1], d["w_f"][:, :-1], d["b_f"], d["w_i"], d["b_i"])["f"] if c["D"] > 1 else
             R.init_lstm_fwd(torch.zeros_like(d["ann"]), *w)["f"], "f without the last feature")
    _noticed(f["init"], f["f"][:, :-1] @ d["w_i"].double()[:, :-1].t() + d["b_i"].double(), "init without the last unit of m")
    for dataset in ("real", "int"):
        di = C.init_inputs(c, i, dataset)
        b = R.init_lstm_bwd(di["dinit"], di["w_f"], di["w_i"], f, c["L"])
        exact = dataset == "int"
        _noticed(b["db_i"], di["dinit"].double()[:-1].sum(0), "db_i without the last row (%s)" % dataset, exact)
        if c["N"] > 1 or not exact:
            _noticed(b["dann"], b["dann"][:-1], "dann without the last row (%s)" % dataset)
        if not exact:
            _noticed(b["df"], di["dinit"].double()[:, :-1] @ di["w_i"].double()[:-1], "df without the last column of dinit")
            _noticed(b["dw_i"], di["dinit"].double()[:-1].t() @ f["f"][:-1], "dw_i without the last row")
            _noticed(b["dw_f"], b["df"][:-1].t() @ f["mean"][:-1], "dw_f without the last row")
            _noticed(b["dann"], b["dann"][:, :-1], "dann without the last location")


@pytest.mark.parametrize("i,c", _ids(C.DS_CASES, C.ds_id))
def test_doubly_stochastic_reference_notices_the_last_element_and_step(i, c):
    a = C.ds_inputs(c, i, "real")
    asum, out = R.doubly_stochastic_fwd(a, c["gamma"])
    less_sum, less_out = R.doubly_stochastic_fwd(a[:, :-1], c["gamma"]) if c["T1"] > 1 else (torch.zeros_like(asum), torch.tensor(c["gamma"] * 1.0))
    _noticed(asum, less_sum, "asum without the last step")
    _noticed(out, less_out, "out without the last step")
    flat = asum.reshape(-1)
    _noticed(flat, flat[:-1], "asum without the last element")
    dal = R.doubly_stochastic_bwd(asum, c["gamma"], c["gscale"], c["T1"]).reshape(-1)
    # the gradient is small by construction (1 / (N L)): it is compared against its own size, not against 1
    assert float(dal[-1].abs()) >= 0.01 * float(dal.abs().max())
    ai = C.ds_inputs(c, i, "int")
    si, oi = R.doubly_stochastic_fwd(ai, c["gamma"])
    _noticed(si.reshape(-1), si.reshape(-1)[:-1], "asum without the last element (int)", True)
    cut = ai.clone(); cut[-1, :, -1] = 0
    _, oc = R.doubly_stochastic_fwd(cut, c["gamma"])
    assert abs(float(oi) - float(oc)) >= 16 * 2.0 ** -24 * float(oi), "out (int) does not notice the last element"
    assert float(((1 - si) ** 2).max()) * 256 < 2 ** 24          # every block partial of ds_rows_kernel is an exact integer


@pytest.mark.parametrize("i,c", _ids(C.SIGMOID_CASES, lambda c: "n%d" % c["n"]))
def test_sigmoid_backward_inputs(i, c):
    for dataset in ("real", "int"):
        dy, y = C.sigmoid_inputs(c, i, dataset)
        ref = R.sigmoid_bwd(dy, y)
        _noticed(ref, ref[:-1], "the last element")
        if dataset == "int":
            assert bool(ref[-1] != 0) and torch.equal(ref.float().double(), ref) and bool((ref * 16 == (ref * 16).round()).all())          # sixteenths: exact in fp32


TOPK = [pytest.param(i, c, id=C.topk_id(i, c)) for i, c in enumerate(C.TOPK_CASES)]


def _knock_out(x, k, taken):
    """k times: the first maximum of what is left, then its place overwritten with `taken`.  The scan starts from best = -inf and
    takes v > best or v == best && i < best_i, which is the first index holding the maximum; NaN never compares."""
    w = np.array(x, dtype=np.float32)
    out = []
    for _ in range(k):
        best = np.nanmax(w) if not np.isnan(w).all() else None
        bi = int(np.flatnonzero(w == best)[0])
        out.append(bi)
        w[bi] = taken
    return out


@pytest.mark.parametrize("i,c", TOPK)
def test_topk_reference_and_the_two_knock_out_rules(i, c):
    x = C.topk_inputs(c, i).numpy()
    n, k = c["n"], c["k"]
    vals, idx = R.ref_topk(x, k)
    assert len(set(idx.tolist())) == k and np.array_equal(vals, x[idx])
    assert all(vals[j] > vals[j + 1] or (vals[j] == vals[j + 1] and idx[j] < idx[j + 1]) for j in range(k - 1))
    rest = np.delete(x, idx)
    assert rest.size == 0 or rest.max() <= vals[-1]
    new = _knock_out(x, k, np.nan)
    assert new == idx.tolist(), "the rule that marks winners apart from -inf is not the stable sort"
    old = _knock_out(x, k, -np.inf)
    # the old rule runs out after the `above` entries greater than -inf: it then takes the lowest index that holds -inf, a place
    # it has taken already when that lies below every -inf of x -- and otherwise a -inf of x, which the knock-out leaves as it is,
    # so that the next pick is the same place again
    above = int((x > -np.inf).sum())
    short = k - above
    if short <= 0:
        assert old == idx.tolist()
    else:
        lowest_inf = int(np.flatnonzero(np.isneginf(x))[0])
        assert old[:above] == idx.tolist()[:above]
        assert (len(set(old)) < k) == (short >= 2 or min(old[:above], default=n) < lowest_inf), (old, idx.tolist())
    if c["kind"] == "exhaust" and c["finite"] == (0, 3):
        assert old == [0, 3, 0, 0] and idx.tolist() == [0, 3, 1, 2]
    if c["kind"] == "random":
        assert n - 1 in idx.tolist()          # the last element is among the winners
    if c["kind"] == "maxima":
        assert idx.tolist()[:2] == sorted(c["at"]) and (np.array(c["at"]) % 1024 // 64).tolist() in ([0, 0], [1, 0])


def test_torch_topk_is_not_the_tie_rule():
    """why ref_topk is a stable sort and not torch.topk: among equal values torch promises no order"""
    x = torch.tensor([3.0, -np.inf, -np.inf, 1.0, -np.inf])
    assert R.ref_topk(x, 4)[1].tolist() == [0, 3, 1, 2]
    assert sorted(torch.topk(x, 4).indices.tolist()[:2]) == [0, 3]


@pytest.mark.parametrize("i,c", _ids(C.BEAM_CASES, C.beam_id))
def test_beam_scores_reference_notices_the_last_word(i, c):
    x, parent = C.beam_inputs(c, i)
    V = c["V"]
    masked = C.beam_masked(c)
    s = R.beam_scores(x, c["T"], masked, parent)
    assert not bool(torch.isnan(s).any()) and bool((torch.isneginf(s) == (torch.isneginf(x) | torch.isin(torch.arange(V), torch.tensor(masked)))).all())
    if V == 1:
        assert float(s[0, 0]) == 0.0
        return
    less = R.beam_scores(x[:, :-1], c["T"], masked, parent)
    fin = torch.isfinite(s[:, :-1]) & torch.isfinite(less)
    for r in range(3):
        full_r, less_r = s[r, :-1][fin[r]], less[r][fin[r]]
        moved, scale = float((full_r - less_r).abs().max()), max(1.0, float(s[r][torch.isfinite(s[r])].abs().max()))
        assert moved >= 100 * TOL * scale, "row %d: the scores move by %.3g < %.3g without the last word" % (r, moved, 100 * TOL * scale)
    assert bool(torch.isneginf(x[1, 0])) and bool(torch.isneginf(x[2, 5::256]).all()) and int(torch.isfinite(x[3]).sum()) == 1
    assert bool(torch.isfinite(x[2, 4::256]).all())
