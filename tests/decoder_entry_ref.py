"""float64 restatements of the decoder's sub-module entry points and search primitives (csrc/decoder_kernels.h behind sat_colsum,
sat_embedding_*, sat_lstm_cell_*, sat_deep_output_*, sat_init_lstm_*, sat_sigmoid_bwd; csrc/decoder_search_kernels.h behind sat_topk and
sat_beam_scores; csrc/ce_loss.hip
behind sat_doubly_stochastic_*), written out with torch double on the CPU, and the frames the GPU tests put their operands in.
tests/decoder_entry_cases.py draws the inputs, test_decoder_entry_ref.py (no GPU) checks these functions against torch's own modules
and the oracle, test_gpu_decoder_entry_points.py compares the kernels with them.

Frames.  An input is a view inside a NaN-filled device buffer: a kernel that reads a row, a column or a padding element it should
not read carries the NaN into its result.  An output or a scratch buffer is a view inside a buffer filled with gemm_ref.CANARY_F32, a
NaN payload no arithmetic produces: what must not be written is still a canary afterwards."""
import numpy as np
import torch

from gemm_ref import CANARY_F32

NAN = float("nan")
GUARD = 64          # elements on either side of every view; a multiple of 4, so a view starts on a 16-byte boundary


def f64(t):
    return None if t is None else t.detach().cpu().double()


# ------------------------------------------------------------------ frames (device side)
def nan_framed(t, off=0, guard=GUARD):
    """fp32 host tensor t as a contiguous view inside a NaN-filled device buffer, `off` floats past a 16-byte boundary, `guard` (a
    multiple of 4) NaN elements on either side"""
    assert guard % 4 == 0
    n = t.numel()
    whole = torch.full((guard + off + n + guard,), NAN, dtype=torch.float32, device="cuda")
    view = whole[guard + off:guard + off + n]
    view.copy_(t.reshape(-1).float())
    assert view.data_ptr() % 16 == (off * 4) % 16
    return whole, view.view(t.shape)


def canary_framed(shape, dtype=torch.float32, inside=None):
    """a 4-byte-element output view inside a canary-filled device buffer; itself canaries, or `inside`"""
    assert dtype in (torch.float32, torch.int32)
    n = int(np.prod(shape)) if len(shape) else 1
    whole = torch.empty(GUARD + n + GUARD, dtype=dtype, device="cuda")
    whole.view(torch.int32).fill_(CANARY_F32)
    view = whole[GUARD:GUARD + n].view(shape)
    if inside is not None:
        view.copy_(inside.to(dtype))
    assert view.data_ptr() % 16 == 0
    return whole, view


def canaries(t):
    return int((t.contiguous().view(torch.int32) == CANARY_F32).sum())


def frame_intact(whole, what):
    assert canaries(whole[:GUARD]) == GUARD and canaries(whole[-GUARD:]) == GUARD, "%s: the frame around it changed" % what


def all_canary(t, what):
    assert canaries(t) == t.numel(), "%s: %d element(s) were written" % (what, t.numel() - canaries(t))


def nan_frame_intact(whole, guard, what):
    assert bool(torch.isnan(whole[:guard]).all()) and bool(torch.isnan(whole[-guard:]).all()), "%s: the frame around the input changed" % what


# ------------------------------------------------------------------ column sums, sigmoid backward, doubly stochastic term
def colsum(x):
    """out[c] = sum_r x[r, c]"""
    return f64(x).sum(0)


def sigmoid_bwd(dy, y):
    dy, y = f64(dy), f64(y)
    return dy * y * (1 - y)


def doubly_stochastic_fwd(alphas, gamma):
    """alphas (N, T1, L) -> (asum (N, L), gamma * mean((1 - asum)^2))"""
    asum = f64(alphas).sum(1)
    return asum, float(np.float32(gamma)) * ((1 - asum) ** 2).mean()


def doubly_stochastic_bwd(asum, gamma, gscale, T1):
    """dalphas (N, T1, L) = gscale * gamma * 2 (asum - 1) / (N L), the same for every t"""
    asum = f64(asum)
    g = (1.0 if gscale is None else float(gscale)) * float(np.float32(gamma)) * 2 * (asum - 1) / asum.numel()
    return g[:, None, :].expand(asum.shape[0], T1, asum.shape[1]).contiguous()


# ------------------------------------------------------------------ embedding
def valid_tokens(tokens, V):
    t = tokens.long()
    return (t >= 0) & (t < V)


def embedding_fwd(table, tokens, max_norm=0.0):
    """nn.Embedding(max_norm) forward: (out (rows, m), the table afterwards).  Rows that occur in `tokens` and whose L2 norm exceeds
    max_norm are rescaled once by max_norm / (norm + 1e-7); an id outside [0, V) gives a zero row."""
    table = f64(table).clone()
    V = table.shape[0]
    ok = valid_tokens(tokens, V)
    if max_norm and max_norm > 0:
        for v in torch.unique(tokens.long()[ok]).tolist():
            norm = float(table[v].norm())
            if norm > max_norm:
                table[v] *= max_norm / (norm + 1e-7)
    out = torch.zeros(tokens.numel(), table.shape[1], dtype=torch.float64)
    out[ok] = table[tokens.long()[ok]]
    return out, table


def embedding_bwd(dY, tokens, V, padding_idx):
    """dtable (V, m): the rows of dY added into the rows of their tokens; ids outside [0, V) and the padding row are skipped"""
    dY = f64(dY)
    t = tokens.long()
    ok = valid_tokens(tokens, V) & (t != padding_idx)
    out = torch.zeros(V, dY.shape[1], dtype=torch.float64)
    out.index_add_(0, t[ok], dY[ok])
    return out


def embedding_bwd_chain_f32(dY, tokens, V, padding_idx):
    """the same in fp32, every table row one chain of additions in increasing row order starting from 0 -- the order
    include/sat_hip.h documents: the kernel must give these bits"""
    dY = dY.detach().cpu().float().numpy()
    t = tokens.long().numpy()
    out = np.zeros((V, dY.shape[1]), np.float32)
    for v in np.unique(t):
        if 0 <= v < V and v != padding_idx:
            out[v] = np.cumsum(dY[t == v], axis=0, dtype=np.float32)[-1]
    return torch.from_numpy(out)


# ------------------------------------------------------------------ LSTM cell (gate order i, f, g, o)
def lstm_cell_fwd(x, h_prev, c_prev, w_ih, w_hh, b_ih, b_hh):
    """-> dict(pre (N, 4n), gates (N, 4n) activated, h_new, c_new)"""
    x, h_prev, c_prev, w_ih, w_hh, b_ih, b_hh = map(f64, (x, h_prev, c_prev, w_ih, w_hh, b_ih, b_hh))
    pre = x @ w_ih.t() + b_ih + h_prev @ w_hh.t() + b_hh
    i, f, g, o = pre.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c_new = f * c_prev + i * g
    return dict(pre=pre, gates=torch.cat([i, f, g, o], 1), c_new=c_new, h_new=o * torch.tanh(c_new))


def lstm_cell_bwd(x, h_prev, c_prev, w_ih, w_hh, fwd, dh_new, dc_new=None):
    """backward of lstm_cell_fwd from its own outputs: dict(dgates, dx, dh_prev, dc_prev, dw_ih, dw_hh, db)"""
    x, h_prev, c_prev, w_ih, w_hh, dh, dcn = map(f64, (x, h_prev, c_prev, w_ih, w_hh, dh_new, dc_new))
    i, f, g, o = fwd["gates"].chunk(4, dim=1)
    tc = torch.tanh(fwd["c_new"])
    dc = dh * o * (1 - tc * tc) + (dcn if dcn is not None else 0)
    dg = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dict(dgates=dg, dx=dg @ w_ih, dh_prev=dg @ w_hh, dc_prev=dc * f, dw_ih=dg.t() @ x, dw_hh=dg.t() @ h_prev, db=dg.sum(0))


# ------------------------------------------------------------------ DeepOutput
def deep_output_fwd(prev_embed, hidden, context, w_h, w_c, w_o, b_o, mask=None):
    """deep (context given): u = tanh(prev_embed + hidden W_h^T + context W_c^T); shallow: u = hidden W_h^T.
    -> dict(u, udrop = u * mask, logits = udrop W_o^T + b_o).  mask (N, m) holds 0 or 1 / (1 - p)."""
    hidden, w_h, w_o = f64(hidden), f64(w_h), f64(w_o)
    u = hidden @ w_h.t()
    if context is not None:
        u = torch.tanh(f64(prev_embed) + u + f64(context) @ f64(w_c).t())
    ud = u if mask is None else u * f64(mask)
    logits = ud @ w_o.t()
    if b_o is not None:
        logits = logits + f64(b_o)
    return dict(u=u, udrop=ud, logits=logits)


def deep_output_bwd(dlogits, hidden, context, w_h, w_c, w_o, fwd, mask=None):
    """-> dict(du (= d_prev_embed in the deep form), d_hidden, d_context, dw_hidden, dw_context, dw_out, db_out)"""
    dl, hidden, w_h, w_o = f64(dlogits), f64(hidden), f64(w_h), f64(w_o)
    du = dl @ w_o
    if mask is not None:
        du = du * f64(mask)
    out = dict(dw_out=dl.t() @ fwd["udrop"], db_out=dl.sum(0))
    if context is not None:
        du = du * (1 - fwd["u"] ** 2)
        out.update(d_context=du @ f64(w_c), dw_context=du.t() @ f64(context))
    out.update(du=du, d_hidden=du @ w_h, dw_hidden=du.t() @ hidden)
    return out


# ------------------------------------------------------------------ InitLSTM
def init_lstm_fwd(ann, w_f, b_f, w_i, b_i, mask=None):
    """ann (N, L, D) -> dict(mean (N, D) after the mask, f (N, m), init (N, n2)).  `init` row-major is the reference's (2 layers, N, n)
    buffer: its reshape has no permute, so there is nothing to restate beyond the two Linear layers."""
    ann, w_f, b_f, w_i, b_i = map(f64, (ann, w_f, b_f, w_i, b_i))
    mean = ann.mean(1)
    if mask is not None:
        mean = mean * f64(mask)
    f = mean @ w_f.t() + b_f
    return dict(mean=mean, f=f, init=f @ w_i.t() + b_i)


def init_lstm_bwd(dinit, w_f, w_i, fwd, L, mask=None):
    """-> dict(dw_i, db_i, df, dw_f, db_f, dmean (after the mask), dann (N, L, D))"""
    dinit, w_f, w_i = map(f64, (dinit, w_f, w_i))
    df = dinit @ w_i
    dmean = df @ w_f
    if mask is not None:
        dmean = dmean * f64(mask)
    return dict(dw_i=dinit.t() @ fwd["f"], db_i=dinit.sum(0), df=df, dw_f=df.t() @ fwd["mean"], db_f=df.sum(0), dmean=dmean,
                dann=(dmean / L)[:, None, :].expand(dmean.shape[0], L, dmean.shape[1]).contiguous())


# ------------------------------------------------------------------ search primitives
def ref_topk(x, k):
    """(values, indices) of the k largest in descending order, equal values in increasing index order, every index once: a stable
    descending sort.  (torch.topk promises no order among ties and does not keep the lowest index.)  -0.0 and +0.0 are equal."""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    idx = np.argsort(-x.astype(np.float64), kind="stable")[:k]
    return x[idx], idx.astype(np.int64)


def beam_scores(logits, temperature, masked, parent):
    """log_softmax(logits / T) + parent in float64, -inf at the masked ids inside [0, V); (rows, V)"""
    x = f64(logits) / float(np.float32(temperature))
    s = torch.log_softmax(x, dim=1)
    if parent is not None:
        s = s + f64(parent)[:, None]
    for v in masked:
        if 0 <= v < x.shape[1]:
            s[:, v] = -float("inf")
    return s
