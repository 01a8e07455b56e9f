"""float64 reference of one attention step (SoftAttention.forward + the beta gate, model.py:94-109, 541) and of its gradients, written from
the formula; the gradients come from float64 autograd through that forward, not from a second derivation.

Layout (that of sat_attention_step_fwd/bwd): N = B * R caption rows, row i belongs to image i // R.
  U (B, L, A) = att_enc(ann);  q (N, A) = att_dec(h);  beta (N, D) = the gate;  wf (A,);  ann (B, L, D);  lengths (N,): row i is live when
  lengths[i] > step.
  e[i, l]  = sum_k wf[k] tanh(U[b, l, k] + q[i, k]) / sqrt(L)
  alpha    = softmax_l(e);  z = alpha . ann[b];  xz = beta * z;  dead rows give zeros everywhere.
For the bf16 annotation stream pass ann rounded to bf16 (bf16_round): the kernels multiply and add in fp32, so the fp32 bound applies."""
import torch

F64 = torch.float64


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _live(lengths, step):
    return (torch.as_tensor(lengths) > step)


def _forward(U, q, beta, wf_img, ann, live, R):
    """wf_img (B, A): one copy of wf per image, so that its gradient is the per-image partial the kernels write"""
    N, L = q.shape[0], U.shape[1]
    img = torch.arange(N) // R
    e = (torch.tanh(U[img] + q[:, None, :]) * wf_img[img][:, None, :]).sum(-1) / float(L) ** 0.5          # (N, L)
    m = live.to(F64)[:, None]
    alpha = torch.softmax(e, dim=1) * m
    z = (alpha[:, :, None] * ann[img]).sum(1)
    return alpha, z, beta * z * m


def forward(U, q, beta, wf, ann, lengths, step, R):
    """-> dict(alphas (N, L), Z (N, D), XZ (N, D)) in float64"""
    U, q, beta, wf, ann = (t.to(F64) for t in (U, q, beta, wf, ann))
    alpha, z, xz = _forward(U, q, beta, wf[None, :].expand(U.shape[0], -1), ann, _live(lengths, step), R)
    return dict(alphas=alpha, Z=z, XZ=xz)


def backward(U, q, beta, wf, ann, lengths, step, R, dZ, dXZ, dalpha=None):
    """External gradients dZ (of z), dXZ (of beta * z) and dalpha (of alpha, or None), all (N, .).  Returns float64
      DZ (N, D)      total gradient of z
      da (N, L)      total gradient of alpha (what the split kernels keep in their scratch); 0 on dead rows
      dq (N, A), dbeta_pre (N, D) = d beta * beta (1 - beta): the gradient of the gate's pre-activation
      dU (B, L, A), dwf_part (B, A): per-image partials of wf's gradient
      dann_context (B, L, D): ann's gradient through z = alpha . ann (alpha held fixed, what sat_attention_context_bwd sums)
    The other term of ann's gradient goes through U = ann W_e^T: dann_scores(dU, W_e)."""
    B = U.shape[0]
    U, q, beta, ann = (t.to(F64).clone().requires_grad_() for t in (U, q, beta, ann))
    wf_img = wf.to(F64)[None, :].expand(B, -1).clone().requires_grad_()
    live = _live(lengths, step)
    alpha, z, xz = _forward(U, q, beta, wf_img, ann, live, R)
    alpha.retain_grad(); z.retain_grad()
    m = live.to(F64)[:, None]
    loss = (z * dZ.to(F64) * m).sum() + (xz * dXZ.to(F64)).sum()
    if dalpha is not None:
        loss = loss + (alpha * dalpha.to(F64) * m).sum()
    loss.backward()
    b = beta.detach()
    # alpha = softmax * mask: the gradient autograd keeps for it is that of the masked product, which is what the kernels call dalpha
    return dict(DZ=z.grad * m, da=alpha.grad * m, dq=q.grad, dbeta_pre=beta.grad * b * (1.0 - b), dU=U.grad, dwf_part=wf_img.grad,
                dann_context=context_bwd(alpha.detach()[:, None, :], (z.grad * m)[None], live.to(torch.int64), R))


def dann_scores(dU, W_e):
    return dU.to(F64) @ W_e.to(F64)


def context_bwd(alphas, DZ, lengths, R, dann0=None):
    """sat_attention_context_bwd as a plain triple sum: alphas (N, T1, L), DZ (T1, N, D) time-major, lengths (N,) ->
    dann[b, l, :] = sum over the image's rows r and steps t < min(lengths, T1) of alphas[i, t, l] * DZ[t, i, :]  (+ dann0)"""
    N, T1, L = alphas.shape
    D = DZ.shape[2]
    out = torch.zeros(N // R, L, D, dtype=F64) if dann0 is None else dann0.to(F64).clone()
    a, g = alphas.to(F64), DZ.to(F64)
    for i in range(N):
        for t in range(min(int(lengths[i]), T1)):
            out[i // R] += a[i, t][:, None] * g[t, i][None, :]
    return out
