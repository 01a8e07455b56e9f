"""GPU: the per-image decoding entry points sat_decoder_infer_begin / sat_decoder_infer_step called on their own through the C ABI
(SAT.beam_decode is their only other caller).  They and the batched searches run one start-up and one step (csrc/decoder_search.hip).

1. begin plus two steps against the oracle's sub-modules (oracle/sat_oracle.py: init_state, embed, soft_attention, beta_gate,
   lstm_step_math, deep_output) in float64: h and c after begin and after the second step, logits and alpha of both steps, within
   1e-4 max(1, max|ref|), the bound tests/test_gpu_decoder_entry_points.py holds the GEMM-backed entry points to.  One and two LSTM
   layers, deep and shallow output, with and without the output bias, beams == max_beams and beams < max_beams, with and without h_noise.
2. begin plus one step at beams == max_beams against the first step of sat_beam_search over that one image (beamk = beams, "beam"
   sampling, max_gen_length 0), bit for bit: alpha is alpha_hist[0]; the search does not return its logits, so they are compared through
   what it makes of them at step 0 with the same kernels SAT.beam_decode uses (sat_beam_scores with the first step's masks, sat_topk
   over row 0): the words in tok_in[1] and their scores in fin_score."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4                                               # tests/test_gpu_decoder_entry_points.py, close()
LC, D, A, M, N, V, KMAX = 4, 8, 8, 8, 8, 16, 3
TOKENS = [3, 7, 1]                                       # what the second step is fed; the first is fed <START>


def _setup(layers, deep, bias, seed=11):
    """(hp, fp32 CPU state dict, annotations (L, D))"""
    from oracle import prng, sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=D, embed_dim=M, attention_dim=A, decoder_dim=N, decoder_layers=layers, deep_output=deep)
    sd = O.random_decoder_state(hp, seed)
    if not bias:
        del sd["output.output.bias"]
    ann = torch.from_numpy(prng.uniform((LC, D), seed + 1, 0.0, 1.0)).float()
    return hp, sd, ann


def _device_params(L, sd, layers, dev):
    from sat_amd import decoder as Dk
    tens = {}
    for name in L.param_names(layers):
        t = sd.get(L.param_key(name))
        tens[name] = None if t is None else t.to(dev).contiguous()
    return Dk._params_struct(tens, layers), tens


def _noise(layers, K, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(layers, K, N, generator=g) * (0.3 / (s + 1)) for s in range(2)]


def _reference(hp, sd, ann, K, toks, noise):
    """model.py:255-327 on the K expanded copies of one image, float64: [(h, c) after begin, (logits, alpha) per step, (h, c) at the end]"""
    from oracle import sat_oracle as O
    sd = {k: v.double() for k, v in sd.items()}
    layers = hp.decoder_layers
    ann4 = ann.double().t().reshape(1, D, LC, 1).expand(K, D, LC, 1)
    h, c = O.init_state(sd, ann4, layers, N)
    out = [(h.clone(), c.clone())]
    for s, tok in enumerate(toks):
        y = O.embed(sd, tok)
        z, alpha = O.soft_attention(sd, ann4, h[-1])
        x = torch.cat([y, O.beta_gate(sd, h[-1]) * z], 1).unsqueeze(0)
        h, c = O.lstm_step_math(sd, x, h if noise is None else h + noise[s].double(), c, layers)
        out.append((O.deep_output(sd, y, h[-1], z, hp.deep_output), alpha.reshape(K, LC)))
    out.append((h, c))
    return out


def _close(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print("%s: max|d| = %.3e (scale %.3g)" % (what, err, scale))
    assert err <= TOL * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, TOL)


class _Infer:
    """one image's begin / step calls on buffers of the test's own"""

    def __init__(self, hp, sd, ann, K):
        import sat_amd  # noqa: F401
        from sat_amd import _lib as L, decoder as Dk
        self.L, self.lib, self.K, self.dev = L, L.lib(), K, torch.device("cuda:0")
        layers = hp.decoder_layers
        self.dims = Dk.decoder_dims(1, KMAX, 2, LC, D, A, M, N, V, 0, hp.deep_output, 0, 0, layers=layers)
        self.w, self.tens = _device_params(L, sd, layers, self.dev)
        self.ann = ann.to(self.dev).contiguous()
        self.ws_bytes = self.lib.sat_decoder_infer_workspace_bytes(C.byref(self.dims), KMAX)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        self.h = torch.full((layers, K, N), float("nan"), device=self.dev)
        self.c = torch.full((layers, K, N), float("nan"), device=self.dev)

    def begin(self):
        L = self.L
        L.check(self.lib.sat_decoder_infer_begin(C.byref(self.dims), C.byref(self.w), L.ptr(self.ann), self.K, KMAX, L.ptr(self.h), L.ptr(self.c), L.ptr(self.ws),
                                                 self.ws_bytes, L.stream_ptr()), "sat_decoder_infer_begin")

    def step(self, tok, noise=None):
        L = self.L
        tok = tok.to(device=self.dev, dtype=torch.int32).contiguous()
        noise = None if noise is None else noise.to(self.dev).contiguous()
        logits = torch.full((self.K, V), float("nan"), device=self.dev)
        alpha = torch.full((self.K, LC), float("nan"), device=self.dev)
        L.check(self.lib.sat_decoder_infer_step(C.byref(self.dims), C.byref(self.w), L.ptr(self.ann), L.ptr(tok), self.K, KMAX, L.ptr(self.h), L.ptr(self.c),
                                                L.ptr(logits), L.ptr(alpha), L.ptr(noise), L.ptr(self.ws), self.ws_bytes, L.stream_ptr()), "sat_decoder_infer_step")
        torch.cuda.synchronize()
        return logits, alpha


CASES = list(itertools.product([1, 2], [True, False], [True, False], [KMAX, KMAX - 1], [False, True]))


@pytest.mark.parametrize("layers,deep,bias,K,noisy", CASES, ids=["layers%d-%s-%s-beams%d-%s" % (l, "deep" if d else "shallow", "bias" if b else "nobias", k,
                                                                                                "noise" if z else "clean") for l, d, b, k, z in CASES])
def test_begin_and_two_steps_against_the_float64_sub_modules(layers, deep, bias, K, noisy):
    hp, sd, ann = _setup(layers, deep, bias)
    start = hp.vocab_stoi["<START>"]
    toks = [torch.full((K,), start, dtype=torch.int64), torch.tensor(TOKENS[:K], dtype=torch.int64)]
    noise = _noise(layers, K, 5) if noisy else None
    ref = _reference(hp, sd, ann, K, toks, noise)
    run = _Infer(hp, sd, ann, K)
    run.begin()
    torch.cuda.synchronize()
    _close(run.h, ref[0][0], "h after begin"); _close(run.c, ref[0][1], "c after begin")
    for s in range(2):
        logits, alpha = run.step(toks[s], None if noise is None else noise[s])
        _close(logits, ref[1 + s][0], "logits of step %d" % s); _close(alpha, ref[1 + s][1], "alpha of step %d" % s)
        assert float((alpha.sum(1) - 1).abs().max()) < 1e-5
    _close(run.h, ref[3][0], "h after two steps"); _close(run.c, ref[3][1], "c after two steps")


@pytest.mark.parametrize("layers,deep,bias", list(itertools.product([1, 2], [True, False], [True, False])))
def test_begin_and_one_step_are_the_first_step_of_the_batched_search_bit_for_bit(layers, deep, bias):
    from sat_amd import decoder as Dk
    hp, sd, ann = _setup(layers, deep, bias)
    K = KMAX
    stoi = hp.vocab_stoi
    run = _Infer(hp, sd, ann, K)
    L, lib, dev = run.L, run.lib, run.dev
    run.begin()
    logits, alpha = run.step(torch.full((K,), stoi["<START>"]))
    # what SAT.beam_decode makes of the first step's logits: masked log-softmax of every row, the top K words of row 0
    masks = torch.tensor([stoi["<START>"], stoi["<PAD>"], stoi["<END>"], stoi["<UNK>"]], dtype=torch.int32, device=dev)
    scores = torch.empty(K, V, device=dev); work = torch.empty(K * V, device=dev)
    vals = torch.empty(K, device=dev); inds = torch.empty(K, dtype=torch.int32, device=dev)
    L.check(lib.sat_beam_scores(L.ptr(logits), K, V, 1.0, L.ptr(masks), 4, None, L.ptr(scores), L.stream_ptr()), "sat_beam_scores")
    L.check(lib.sat_topk(L.ptr(scores), L.ptr(work), V, K, L.ptr(vals), L.ptr(inds), L.stream_ptr()), "sat_topk")
    # the batched search of that one image, cut after its first step: every kept hypothesis is recorded as it stands
    desc = Dk.search_desc(stoi, K, 0, 1.0, dev)
    desc.d, desc.w, desc.ann = C.pointer(run.dims), C.pointer(run.w), run.ann.data_ptr()
    o = Dk.beam_search(desc, 1, LC, dev)
    torch.cuda.synchronize()

    def bits(t):
        return t.detach().contiguous().view(torch.int32).cpu()
    assert torch.equal(bits(o["alpha_hist"][0, 0]), bits(alpha)), "alpha of the first step differs from alpha_hist[0]"
    assert int(o["fin_count"][0]) == K
    assert torch.equal(o["tok_in"][1, 0].cpu(), inds.cpu()), "the first step's words differ"
    assert torch.equal(bits(o["fin_score"][0]), bits(vals)), "the first step's scores differ"
