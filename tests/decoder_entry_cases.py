"""The shapes at which the decoder's sub-module entry points and search primitives are pinned (csrc/decoder_kernels.h, csrc/decoder_search_kernels.h, and csrc/ce_loss.hip
for the doubly-stochastic term, behind the sat_* names below), one table per entry point: the smallest shapes at which each loop, guard and branch of the kernels differs, each
with the path it must take and why it is there.  test_decoder_entry_ref.py (no GPU) checks that the inputs drawn here make the
float64 reference of tests/decoder_entry_ref.py notice a dropped last row, column, token occurrence or time step;
test_gpu_decoder_entry_points.py runs them.

Data sets.  "real": standard normals (the last row / column / unit enlarged where the sensitivity check needs it), compared within
1e-4 max(1, max|ref|).  "int": small integers as fp32, |x| <= 8 and at most 2^15 terms, so every partial sum is exact in any order
and the result must equal the reference bit for bit."""
import torch

import decoder_entry_ref as R

EMB_LIST = 1024          # csrc/decoder_kernels.h: tokens one block sorts in LDS; more take the scanning path
NEG_INF = float("-inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ------------------------------------------------------------------ sat_colsum
# colsum_part4_kernel (128 threads x 4 columns, rows unrolled by 4) when cols % 4 == 0, ld % 4 == 0 and x is 16-byte aligned,
# else colsum_part_kernel (256 threads); parts of 256 rows, colsum_finish_kernel adds the parts in order.
def _cs(rows, cols, path, why, ld=None, off=0):
    return dict(rows=rows, cols=cols, ld=ld or cols, off=off, path=path, why=why)


COLSUM_CASES = [
    _cs(1, 36, "vec", "one row: only the row tail loop"),
    _cs(3, 36, "vec", "three rows: the tail loop alone, three trips"),
    _cs(4, 36, "vec", "one unrolled trip, no tail"),
    _cs(5, 36, "vec", "one unrolled trip and one tail row"),
    _cs(255, 36, "vec", "one part, short by a row: 63 unrolled trips + 3 tail rows"),
    _cs(256, 36, "vec", "exactly one part"),
    _cs(257, 36, "vec", "a second part of one row"),
    _cs(513, 36, "vec", "three parts, the last of one row"),
    _cs(5, 4, "vec", "one live thread"),
    _cs(257, 4, "vec", "one live thread, two parts"),
    _cs(5, 512, "vec", "512 columns fill one 128-thread block exactly"),
    _cs(257, 512, "vec", "the same with two parts"),
    _cs(5, 516, "vec", "a second block with one live thread"),
    _cs(257, 516, "vec", "the same with two parts"),
    _cs(257, 36, "vec", "ld = cols + 4: the padding columns are NaN", ld=40),
    _cs(5, 4, "vec", "ld = 8: one live thread next to NaN padding", ld=8),
    _cs(1, 1, "scalar", "smallest"),
    _cs(513, 1, "scalar", "one column, three parts"),
    _cs(1, 23, "scalar", "the toy width, one row"),
    _cs(3, 23, "scalar", "the toy width, three rows"),
    _cs(256, 23, "scalar", "exactly one part"),
    _cs(257, 23, "scalar", "a second part of one row"),
    _cs(513, 23, "scalar", "three parts"),
    _cs(5, 257, "scalar", "a second 256-thread block with one live thread"),
    _cs(257, 257, "scalar", "the same with two parts"),
    _cs(4, 36, "scalar", "ld = 37: cols % 4 == 0 alone does not allow 16-byte loads", ld=37),
    _cs(257, 36, "scalar", "ld = 37, two parts", ld=37),
    _cs(5, 36, "scalar", "x one float past a 16-byte boundary", off=1),
    _cs(513, 36, "scalar", "x one float past a 16-byte boundary, three parts", off=1),
]


def colsum_id(c):
    return "r%d-c%d-ld%d%s-%s" % (c["rows"], c["cols"], c["ld"], "-off" if c["off"] else "", c["path"])


def colsum_path(c):
    """the path csrc/decoder.hip: colsum takes for the case (the test allocates x `off` floats past a 16-byte boundary)"""
    return "vec" if c["cols"] % 4 == 0 and c["ld"] % 4 == 0 and c["off"] % 4 == 0 else "scalar"


def colsum_inputs(c, index, dataset):
    """x (rows, cols).  The last row holds +-max(1, 5% of the largest partial sum) and the last column sums to at least 5% of the
    largest sum (int: the last row is never 0, the last column's sum neither): the result notices either one missing."""
    g = _gen(1000 + index)
    rows, cols = c["rows"], c["cols"]
    x = _ints(g, -8, 8, rows, cols) if dataset == "int" else torch.randn(rows, cols, generator=g)
    big = max(1.0, 0.05 * float(x[:rows - 1].sum(0).abs().max())) if rows > 1 else 1.0
    if dataset == "int":
        big = float(min(8, int(big)))
    x[rows - 1] = big * torch.where(torch.arange(cols) % 2 == 0, 1.0, -1.0)
    if rows > 1:
        s = x.double().sum(0)
        need = 1.0 if dataset == "int" else 0.05 * float(s.abs().max())
        if abs(float(s[cols - 1])) < need:
            x[0, cols - 1] = x[0, cols - 1] - float(s[cols - 1]) + (need if dataset != "int" else (1.0 if x[0, cols - 1] < 8 else -1.0))
    return x


# ------------------------------------------------------------------ sat_embedding_bwd
# count / scan (1024 threads, ceil(V / 1024) rows each) / place / sum.  A vocabulary row with up to EMB_LIST tokens sorts its
# segment (bitonic, padded to a power of two); one with more scans the token array in chunks of 256 and flushes its list whenever the
# next chunk might not fit.  `plan`: (token, occurrences, stride) placed from row 0 on, stride 1 = every row, 2 = every second row;
# `fill`: what the rows left over hold, cycled.
def _eb(V, m, pad, rows, plan, fill, why):
    return dict(V=V, m=m, pad=pad, rows=rows, plan=plan, fill=fill, why=why)


EMB_BWD_CASES = [
    _eb(1025, 1, 0, 300, [(5, 1, 1), (6, 2, 1), (7, 3, 1), (1024, 1, 1)], [-1, 1025, 1028, 0, 9, 10, 11],
        "sorted path: 0, 1, 2 and 3 occurrences (3 pads to 4), the last id, ids >= V and -1 skipped, the padding row 0 used and zeroed; "
        "V = 1025: 2 rows per scan thread, the ranges of threads 513.. start past V; 300 rows: second block short"),
    _eb(1024, 255, -1, 2052, [(3, 1023, 2), (1023, 1024, 2)], [-1, 1024],
        "sorted path at its limit: 1023 (pads to 1024) and 1024 = EMB_LIST occurrences, interleaved; V = 1024: one row per scan thread; no padding row"),
    _eb(1, 256, -1, 1025, [(0, 1025, 1)], [-1],
        "scanning path, one flush exactly at the boundary (4 full chunks = 1024) and one occurrence left; V = 1: the ranges of threads 1.. start past V"),
    _eb(1024, 257, 0, 1290, [(7, 1280, 1)], [0, -1, 2000, 8],
        "scanning path, dense: one flush of 1024 and a last list of 256; padding row 0 used; m = 257: second trip of one column"),
    _eb(2049, 1, -1, 2563, [(4, 1280, 2), (2048, 1280, 2)], [-1, 2049, 1],
        "scanning path, sparse: the token on every second row, 128 hits a chunk, flushes of 896 < EMB_LIST; V = 2049: 3 rows per scan thread; 2563 rows"),
    _eb(2049, 4, 0, 2065, [(2048, 2056, 1)], [-1, 0, 2052, 3],
        "scanning path: 2049 + 7 occurrences, flushes at 1024 and 2048 and a partial last chunk of 8"),
]


def emb_bwd_id(c):
    return "V%d-m%d-pad%d-rows%d" % (c["V"], c["m"], c["pad"], c["rows"])


def emb_bwd_tokens(c):
    rows = c["rows"]
    FREE = -7
    tok = torch.full((rows,), FREE, dtype=torch.int32)
    for t, count, stride in c["plan"]:
        free = [r for r in range(rows) if int(tok[r]) == FREE]
        pos = free[:count] if stride == 1 else list(range(free[0], rows, stride))[:count]
        assert len(pos) == count and all(int(tok[r]) == FREE for r in pos), (t, count)
        tok[pos] = t
    free = [r for r in range(rows) if int(tok[r]) == FREE]
    for j, r in enumerate(free):
        tok[r] = c["fill"][j % len(c["fill"])]
    return tok


def emb_bwd_inputs(c, index, dataset):
    """(tokens, dY).  int: integers in -8 .. 8, never 0: every occurrence, the last one included, moves its sum by at least 1.
    real: normals, the last column doubled, and the row of the last occurrence of every token of the plan holds +-(1 + 2% of the
    largest gradient)."""
    g = _gen(2000 + index)
    tok = emb_bwd_tokens(c)
    if dataset == "int":
        dY = _ints(g, -8, 8, c["rows"], c["m"])
        dY[dY == 0] = 1.0
        return tok, dY
    dY = torch.randn(c["rows"], c["m"], generator=g)
    dY[:, c["m"] - 1] *= 2
    big = 1 + 0.02 * float(R.embedding_bwd(dY, tok, c["V"], c["pad"]).abs().max())
    for t, _, _ in c["plan"]:
        r = int(torch.nonzero(tok == t)[-1])
        dY[r] = big * torch.where(torch.arange(c["m"]) % 2 == 0, 1.0, -1.0)
    return tok, dY


def occurrences(tok, V, pad):
    """token -> number of rows that count for its gradient"""
    out = {}
    for t in tok.tolist():
        if 0 <= t < V and t != pad:
            out[t] = out.get(t, 0) + 1
    return out


# ------------------------------------------------------------------ sat_embedding_fwd
# gather_rows_kernel: one block of 64 threads per token.  V = 11; tokens: 2 three times (rescaled once), -1, V and V + 3 (zero
# rows), 5 and 7 (norm below max_norm: untouched), 10 = the last id (rescaled).  Rows 0, 1, 3, 4, 6, 8, 9 are not used.
EMB_FWD_V = 11
EMB_FWD_TOKENS = [2, -1, 5, 2, EMB_FWD_V, 7, EMB_FWD_V + 3, 2, 10]
EMB_FWD_CASES = [
    dict(m=1, max_norm=1.0, why="one column: the norm is |x|"),
    dict(m=63, max_norm=1.0, why="one short trip of the 64 threads"),
    dict(m=64, max_norm=1.0, why="exactly one trip"),
    dict(m=65, max_norm=1.0, why="a second trip of one thread"),
    dict(m=300, max_norm=1.0, why="five trips, the last short"),
    dict(m=65, max_norm=0.0, why="max_norm off: no flags scratch, the table is only read"),
]
EMB_FWD_BIG, EMB_FWD_SMALL = (2, 10, 3, 9), (5, 7, 0, 6)          # rows of norm 3 (3 and 9 unused), rows of norm 1/2; the rest norm 2


def emb_fwd_id(c):
    return "m%d-maxnorm%g" % (c["m"], c["max_norm"])


def emb_fwd_inputs(c, index):
    g = _gen(3000 + index)
    table = torch.randn(EMB_FWD_V, c["m"], generator=g)
    table[:, c["m"] - 1] = table[:, c["m"] - 1].abs() + 0.5
    norm = table.double().norm(dim=1, keepdim=True)
    want = torch.full((EMB_FWD_V, 1), 2.0, dtype=torch.float64)
    want[list(EMB_FWD_BIG)] = 3.0
    want[list(EMB_FWD_SMALL)] = 0.5
    return (table.double() * want / norm).float(), torch.tensor(EMB_FWD_TOKENS, dtype=torch.int32)


# ------------------------------------------------------------------ sat_lstm_cell_fwd / sat_lstm_cell_bwd
# two GEMMs + lstm_cell_fwd_kernel (one thread per (row, unit), 256 a block); backward: the cell kernel, four GEMMs and the column
# sum of dgates (4 n columns: always the vector path).
def _lc(N, n, inp, dc, variant, why, seed=0):
    return dict(N=N, n=n, inp=inp, dc=dc, variant=variant, why=why, seed=seed)


LSTM_CASES = [
    _lc(15, 17, 5, True, "real", "N n = 255: one block, one idle thread"),
    _lc(16, 16, 8, False, "real", "N n = 256: exactly one block"),
    _lc(257, 1, 3, True, "real", "N n = 257: a second block of one thread; n = 1; two column-sum parts", seed=5),          # n = 1: the last row is one unit; this draw leaves none of its outputs near 0
    _lc(5, 9, 22, False, "real", "the toy shape of test_gpu_modules.py: 4 n = 36 takes the vector column sum"),
    _lc(300, 12, 7, False, "real", "two column-sum parts, 15 blocks"),
    _lc(15, 17, 5, True, "saturating", "pre-activations to +-40 and +-200, c_prev to +-30: gates of exactly 0 and 1"),
    _lc(5, 9, 22, False, "saturating", "the same without dc_new"),
    _lc(16, 16, 8, False, "tiny", "pre-activations of order 1e-4: tanh near 0, where 1 - 2 / (e + 1) has no relative accuracy"),
]


def lstm_id(c):
    return "N%d-n%d-in%d-%s%s" % (c["N"], c["n"], c["inp"], c["variant"], "-dc" if c["dc"] else "")


def lstm_inputs(c, index):
    """real: pre-activations of standard deviation ~1.5; the last input column and the last hidden unit weigh 3 times the others, the
    last row's dh (and dc_new) is +-4.
    saturating: pre-activations of standard deviation ~100, c_prev uniform in +-30.  tiny: weights and biases scaled to 1e-4."""
    g = _gen(4000 + index + 100 * c["seed"])
    N, n, inp, v = c["N"], c["n"], c["inp"], c["variant"]
    r = lambda *s: torch.randn(*s, generator=g)
    scale = {"real": 1.0, "saturating": 70.0, "tiny": 1e-4}[v]
    d = dict(x=r(N, inp), h=r(N, n), c=r(N, n), w_ih=r(4 * n, inp) * scale / inp ** 0.5, w_hh=r(4 * n, n) * scale / n ** 0.5,
             b_ih=r(4 * n) * 0.5 * scale, b_hh=r(4 * n) * 0.5 * scale, dh=r(N, n), dc=r(N, n) if c["dc"] else None)
    if v == "real":
        d["w_ih"][:, inp - 1] *= 3
        d["w_hh"][:, n - 1] *= 3
        d["dh"][N - 1] = 4 * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
        if c["dc"]:
            d["dc"][N - 1] = d["dh"][N - 1]
    elif v == "saturating":
        d["c"] = (torch.rand(N, n, generator=g) * 2 - 1) * 30
    else:
        d["c"] = d["c"] * 1e-4
    return d


# ------------------------------------------------------------------ sat_deep_output_fwd / sat_deep_output_bwd
# GEMMs (tanh epilogue in the deep form), dropout_rows_kernel, the column sum of dlogits over V (db_out).
def _do(N, m, n, D, V, deep, p, db, why):
    return dict(N=N, m=m, n=n, D=D, V=V, deep=deep, p=p, db=db, why=why)


DEEP_CASES = [
    _do(5, 10, 9, 12, 23, True, 0.0, True, "deep, V = 23: scalar column sum of dlogits"),
    _do(5, 10, 9, 12, 24, True, 0.4, True, "deep with dropout, V = 24: vector column sum"),
    _do(5, 10, 9, 12, 23, False, 0.4, False, "shallow with dropout, db_out NULL (tied weights): d_prev_embed is the work buffer"),
    _do(5, 10, 9, 12, 24, False, 0.0, True, "shallow, V = 24"),
    _do(5, 10, 9, 12, 24, True, 0.0, False, "deep, db_out NULL"),
    _do(257, 10, 9, 12, 1003, True, 0.0, True, "N = 257, V = 1003: two column-sum parts, four scalar column blocks, the last of 235"),
    _do(128, 32, 9, 12, 24, False, 0.4, True, "N m = 4096: the kept fraction of the dropout mask"),
]


def deep_id(c):
    return "N%d-m%d-V%d-%s-p%g%s" % (c["N"], c["m"], c["V"], "deep" if c["deep"] else "shallow", c["p"], "" if c["db"] else "-nodb")


def deep_inputs(c, index, dataset="real"):
    """the last unit of m, n and D weighs 3 times the others; int: dlogits integers in -8 .. 8 (db_out exact)"""
    g = _gen(5000 + index)
    N, m, n, D, V = c["N"], c["m"], c["n"], c["D"], c["V"]
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(prev=r(N, m) * 0.5, hidden=r(N, n), context=r(N, D), w_h=r(m, n) / n ** 0.5, w_c=r(m, D) / D ** 0.5 * 0.5, w_o=r(V, m) / m ** 0.5,
             b_o=r(V), dlogits=_ints(g, -8, 8, N, V) if dataset == "int" else r(N, V))
    d["w_h"][:, n - 1] *= 3; d["w_c"][:, D - 1] *= 3; d["w_o"][:, m - 1] *= 3
    if dataset == "int":
        d["dlogits"][N - 1][d["dlogits"][N - 1] == 0] = 1.0
        if float(d["dlogits"][:, V - 1].sum()) == 0:
            d["dlogits"][0, V - 1] += 1.0 if d["dlogits"][0, V - 1] < 8 else -1.0
    else:          # the last word's column sums to at least a tenth of the largest column sum
        s = d["dlogits"].double().sum(0)
        if abs(float(s[V - 1])) < 0.1 * float(s.abs().max()):
            d["dlogits"][0, V - 1] += 0.1 * float(s.abs().max()) - float(s[V - 1])
    return d


# ------------------------------------------------------------------ sat_init_lstm_fwd / sat_init_lstm_bwd
# ann_mean_kernel (one block per row, L sequential additions), init_mean_rows_kernel (dropout), two GEMMs; backward: GEMMs, the
# column sums of dinit (n2 columns) and df (m columns), dann_add_mean_kernel.
def _il(N, L, D, m, n2, p, why):
    return dict(N=N, L=L, D=D, m=m, n2=n2, p=p, why=why)


INIT_CASES = [
    _il(1, 1, 1, 1, 2, 0.0, "smallest"),
    _il(1, 1, 1, 1, 2, 0.3, "smallest with dropout: one mask element"),
    _il(5, 49, 12, 10, 36, 0.0, "the toy shape: 7x7 map; n2 = 36 vector column sum, m = 10 scalar"),
    _il(5, 49, 12, 10, 36, 0.3, "the same with dropout"),
    _il(300, 4, 257, 9, 18, 0.0, "two column-sum parts; D = 257: a second trip of one thread in the mean; L = 4: dann exact for integers"),
    _il(300, 4, 257, 9, 18, 0.3, "the same with dropout: 77100 mask elements, the kept fraction"),
]


def init_id(c):
    return "N%d-L%d-D%d-m%d-n%d-p%g" % (c["N"], c["L"], c["D"], c["m"], c["n2"], c["p"])


def init_inputs(c, index, dataset="real"):
    """real: the last location is 3 + |normal| (it moves the mean), the last feature and the last unit of m weigh 3 times the others.
    int: dinit, w_f and w_i integers in -2 .. 2: df, dmean, the bias gradients and (L a power of two) dann are exact."""
    g = _gen(6000 + index)
    N, L, D, m, n2 = c["N"], c["L"], c["D"], c["m"], c["n2"]
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(ann=r(N, L, D), w_f=r(m, D) / D ** 0.5, b_f=r(m) * 0.5, w_i=r(n2, m) / m ** 0.5, b_i=r(n2) * 0.5, dinit=r(N, n2))
    d["ann"][:, L - 1] = (d["ann"][:, L - 1].abs() + 3) * L
    d["w_f"][:, D - 1] *= 3; d["w_i"][:, m - 1] *= 3
    if dataset == "int":
        d["dinit"], d["w_f"], d["w_i"] = _ints(g, -2, 2, N, n2), _ints(g, -2, 2, m, D), _ints(g, -2, 2, n2, m)
        d["dinit"][N - 1][d["dinit"][N - 1] == 0] = 1.0
    return d


# ------------------------------------------------------------------ sat_doubly_stochastic_fwd / sat_doubly_stochastic_bwd
# ds_rows_kernel: one thread per (row, location), T1 sequential additions, a 256-wide tree per block; ds_finish_kernel: 256 threads
# over the block partials in double; ds_grad_kernel: one thread per element of dalphas.
def _ds(N, L, T1, gscale, why):
    return dict(N=N, L=L, T1=T1, gscale=gscale, gamma=0.7, why=why)


DS_CASES = [
    _ds(5, 51, 1, None, "N L = 255: one block, one idle thread; one step"),
    _ds(16, 16, 9, 0.25, "N L = 256: exactly one block"),
    _ds(257, 1, 9, None, "N L = 257: a second block of one thread; L = 1"),
    _ds(350, 200, 1, 3.0, "N L = 70000: 274 blocks, ds_finish_kernel's second trip"),
    _ds(350, 200, 9, None, "the same with nine steps"),
]


def ds_id(c):
    return "N%d-L%d-T%d-%s" % (c["N"], c["L"], c["T1"], "g" if c["gscale"] is not None else "nog")


def ds_inputs(c, index, dataset):
    """real: uniform in (0, 1), the last step in (1, 2).  int: integers 0 .. 2, the last (row, location) 8 at every step: the mean
    of (1 - sum)^2 notices it."""
    g = _gen(7000 + index)
    N, L, T1 = c["N"], c["L"], c["T1"]
    if dataset == "int":
        a = _ints(g, 0, 2, N, T1, L)
        a[N - 1, :, L - 1] = 8.0
    else:
        a = torch.rand(N, T1, L, generator=g)
        a[:, T1 - 1] += 1.0
    return a


# ------------------------------------------------------------------ sat_sigmoid_bwd
SIGMOID_CASES = [dict(n=1, why="one element"), dict(n=256, why="exactly one block"), dict(n=257, why="a second block of one thread")]


def sigmoid_inputs(c, index, dataset):
    """int: dy integers in -8 .. 8 (never 0), y in {1/4, 1/2, 3/4} and 0 and 1 in the first two places: dy y (1 - y) is exact"""
    g = _gen(8000 + index)
    n = c["n"]
    if dataset == "int":
        dy = _ints(g, -8, 8, n); dy[dy == 0] = 3.0
        y = (torch.randint(1, 4, (n,), generator=g).float()) / 4
        if n > 2:
            y[0], y[1] = 0.0, 1.0
        return dy, y
    dy = torch.randn(n, generator=g); dy[n - 1] = 4.0
    y = torch.sigmoid(torch.randn(n, generator=g)); y[n - 1] = 0.5
    return dy, y


# ------------------------------------------------------------------ sat_topk
# one block of 1024 threads: thread t scans i = t, t + 1024, ...; 64-lane butterfly, 16 wave results, thread 0 decides.
def _tk(n, k, kind, why, **kw):
    return dict(n=n, k=k, kind=kind, why=why, **kw)


TOPK_CASES = [
    _tk(1, 1, "random", "one element"),
    _tk(63, 1, "random", "one wave, one idle lane"), _tk(63, 5, "random", "k = 5"), _tk(63, 63, "random", "k = n: a full sort"),
    _tk(64, 1, "random", "exactly one wave"), _tk(64, 5, "random", "k = 5"), _tk(64, 64, "random", "k = n"),
    _tk(65, 1, "random", "a second wave of one lane"), _tk(65, 5, "random", "k = 5"), _tk(65, 65, "random", "k = n"),
    _tk(1023, 5, "random", "one idle thread"), _tk(1024, 5, "random", "every thread one element"),
    _tk(1025, 5, "random", "thread 0 has a second trip; the last element is the maximum"), _tk(50000, 5, "random", "49 trips"),
    _tk(65, 65, "ties", "integers in 0 .. 3: long runs of equal values, in index order"),
    _tk(1025, 5, "ties", "the same over two trips"),
    _tk(65, 65, "equal", "all equal: the indices 0 .. n - 1 in order"),
    _tk(1025, 5, "equal", "all equal over two trips"),
    _tk(64, 3, "maxima", "equal maxima in two lanes of one wave", at=(7, 3)),
    _tk(1024, 3, "maxima", "equal maxima in two waves", at=(74, 10)),
    _tk(1100, 3, "maxima", "equal maxima in the two trips of one thread", at=(1030, 6)),
    _tk(5, 4, "zeros", "+0.0 and -0.0 are equal: index order decides"),
    _tk(200, 6, "zeros", "the same across waves"),
    _tk(65, 5, "exhaust", "exactly k entries above -inf", finite=(64, 0, 13, 40, 63)),
    _tk(5, 4, "exhaust", "fewer than k: x = [3, -inf, -inf, 1, -inf] gives 0, 3, 1, 2", finite=(0, 3)),
    _tk(1025, 5, "exhaust", "fewer than k, the finite ones at 1024 (second trip) and 3: the rest is 0, 1, 2", finite=(1024, 3)),
    _tk(65, 65, "exhaust", "k = n with three finite entries: every -inf index once", finite=(64, 2, 33)),
    _tk(65, 5, "exhaust", "all -inf: 0 .. 4", finite=()),
    _tk(1025, 3, "exhaust", "all -inf over two trips", finite=()),
]


def topk_id(i, c):
    return "%02d-n%d-k%d-%s" % (i, c["n"], c["k"], c["kind"])


def topk_inputs(c, index):
    g = _gen(9000 + index)
    n, kind = c["n"], c["kind"]
    if kind == "random":
        x = torch.randn(n, generator=g)
        x[n - 1] = 9.0 + index                  # the last element is the winner: a scan that stops short loses it
    elif kind == "ties":
        x = _ints(g, 0, 3, n); x[n - 1] = 3.0
    elif kind == "equal":
        x = torch.full((n,), -1.5)
    elif kind == "maxima":
        x = torch.randn(n, generator=g).clamp_(-3, 3)
        for i in c["at"]:
            x[i] = 7.0
    elif kind == "zeros":
        x = torch.full((n,), -1.0)
        for j, i in enumerate(range(0, n, max(1, n // 5))):
            x[i] = -0.0 if j % 2 == 0 else 0.0
        x[n - 1] = -0.0
    else:
        x = torch.full((n,), NEG_INF)
        for j, i in enumerate(c["finite"]):
            x[i] = 3.0 - j
    return x


# ------------------------------------------------------------------ sat_beam_scores
# one block of 256 threads per row: thread t reads v = t, t + 256, ...; online max / sum, butterfly, four wave results.
# Rows: 0 plain; for V >= 255 also 1: -inf at position 0, 2: -inf at every position thread 5 reads, 3: -inf everywhere except V // 2.
def _bs(V, T, parent, why):
    return dict(V=V, T=T, parent=parent, why=why)


BEAM_CASES = [
    _bs(1, 1.0, False, "one word: the score is 0"),
    _bs(255, 0.7, True, "one idle thread"),
    _bs(256, 1.0, True, "every thread one word"),
    _bs(257, 0.7, False, "thread 0 has a second trip"),
    _bs(10000, 1.0, False, "40 trips, the last short"),
    _bs(10000, 0.7, True, "the same with temperature and parent scores"),
]


def beam_id(c):
    return "V%d-T%g-%s" % (c["V"], c["T"], "parent" if c["parent"] else "noparent")


def beam_masked(c):
    """device ids to mask: two inside (when V allows), three outside [0, V)"""
    V = c["V"]
    return ([1, V - 2] if V > 4 else []) + [-1, V, V + 5]


def beam_inputs(c, index):
    """logits 3 * normal, the last one 2 above the logsumexp of the others at the row's temperature (it holds most of the mass: the
    scores notice it missing); parent scores in (-20, 0)"""
    g = _gen(10000 + index)
    V, T = c["V"], c["T"]
    rows = 4 if V >= 255 else 1
    x = torch.randn(rows, V, generator=g) * 3
    if rows == 4:
        x[1, 0] = NEG_INF
        x[2, 5::256] = NEG_INF
        keep = float(x[3, V // 2])
        x[3] = NEG_INF
        x[3, V // 2] = keep
    if V > 1:
        for r in range(min(rows, 3)):
            x[r, V - 1] = float(torch.logsumexp(x[r, :V - 1].double() / T, 0)) * T + 2 * T
    parent = -torch.rand(rows, generator=g) * 20 if c["parent"] else None
    return x, parent
