"""The shapes at which each launch form of the attention step is pinned, each with the plan it was written for (csrc/decoder.hip:
attention_plan).  test_attention_plan.py (no GPU) asserts that sat_attention_step_plan returns exactly these plans and that the inputs
drawn here make the float64 reference sensitive to every last location, unit, feature and caption row; test_gpu_attention_forms.py
runs them.

Step cases: dict(op, R, L, D, A, hc_ld, scratch, ann_off, plan, why).  B is 3 throughout.  `scratch`: a score scratch is passed to the
forward (the backward always has its dalpha scratch).  `ann_off`: ann starts this many floats past a 16-byte boundary.
plan = (form, RN, passes, VW, dchunk, LDS bytes of the scores | dalpha | single kernel, LDS bytes of the context | tanh kernel);
form 0 = the split pair, 1 = one launch.  LDS sizes, in floats:
  forward split   scores RN A + A;  context ceil4(RN L) + 4 * 16 RN 16
  forward single  8 L + 8 A + A + 8 * 256 VW
  backward split  dalpha RN D;  tanh RN L + 32 RN + 32 (RN + 1) 32
  backward single 16 L + 8 A + A + 8 D + 16 * 8 A + 16 A
Context-backward cases: dict(R, L, D, T1, accumulate, plan = (NQ, Lq, LDS bytes = R T1 Lq 16), why)."""
import torch

B = 3
SPLIT, SINGLE = 0, 1
FLAG_SCRATCH, FLAG_ANN_ALIGNED, FLAG_ROWS_ALIGNED, FLAG_BF16 = 1, 2, 4, 8
OPS = {"fwd": 0, "bwd": 1, "ctx": 2}


def _c(op, R, L, D, A, plan, why, hc_ld=None, scratch=True, ann_off=0, dalphas=True, dhc_pad=0):
    return dict(op=op, R=R, L=L, D=D, A=A, hc_ld=hc_ld or A + D, scratch=scratch, ann_off=ann_off, dalphas=dalphas, dhc_pad=dhc_pad, plan=plan, why=why)


STEP_CASES = [
    # ---- forward, split pair (fp32 and bf16 annotation stream)
    _c("fwd", 1, 5, 4, 4, (SPLIT, 1, 1, 4, 64, 32, 4128), "smallest split: one vector, one row, 15 idle vector lanes"),
    _c("fwd", 5, 49, 72, 128, (SPLIT, 5, 1, 4, 64, 3072, 21472), "second 64-wide slice holds 2 vectors; k loop of two trips"),
    _c("fwd", 8, 196, 64, 64, (SPLIT, 8, 1, 4, 64, 2304, 39040), "softmax and context loops over several trips, 196 = 3 * 64 + 4, short last score block"),
    _c("fwd", 9, 17, 8, 68, (SPLIT, 8, 2, 4, 64, 2448, 33312), "passes 8 + 1, one live wave in the second score block, partial second k trip"),
    _c("fwd", 17, 64, 128, 32, (SPLIT, 8, 3, 4, 64, 1152, 34816), "three passes"),
    _c("fwd", 3, 6, 8, 4, (SPLIT, 3, 1, 4, 64, 64, 12368), "hc_ld = A + D + 8: the gate and q are read with the row stride, not A + D", hc_ld=20),
    # ---- forward, one launch, 16-byte annotation loads (no scratch)
    _c("fwd", 2, 7, 12, 8, (SINGLE, 2, 1, 4, 12, 33280, 0), "3 vectors, 4 location groups", scratch=False),
    _c("fwd", 3, 9, 260, 4, (SINGLE, 3, 1, 4, 256, 33200, 0), "chunks 256 + 4", scratch=False),
    _c("fwd", 9, 5, 8, 4, (SINGLE, 8, 2, 4, 8, 33072, 0), "R = 9: two passes", scratch=False),
    # ---- forward, one launch, scalar annotation loads (the scratch is passed and must stay untouched)
    _c("fwd", 3, 5, 10, 7, (SINGLE, 3, 1, 1, 10, 8604, 0), "D % 4 != 0 and an odd hc_ld", hc_ld=19),
    _c("fwd", 2, 6, 70, 8, (SINGLE, 2, 1, 1, 64, 8672, 0), "chunks 64 + 6"),
    _c("fwd", 2, 5, 12, 8, (SINGLE, 2, 1, 1, 12, 8640, 0), "ann 4 bytes past a 16-byte boundary", ann_off=1),
    _c("fwd", 2, 5, 8, 6, (SINGLE, 2, 1, 4, 8, 33144, 0), "A % 4 alone leaves the split pair; D and ann still allow 16-byte loads, so VW stays 4"),
    # ---- backward, split pair (fp32 and bf16 annotation stream)
    _c("bwd", 1, 5, 4, 4, (SPLIT, 1, 1, 4, 0, 16, 8340), "smallest: D = 4, R = 1, one lane of the dalpha loop"),
    _c("bwd", 5, 16, 72, 7, (SPLIT, 5, 1, 4, 0, 1440, 25536), "D = 72 (18 of 64 lanes), A = 7, L = 16: exactly one dalpha block", dalphas=False, dhc_pad=3),
    _c("bwd", 2, 17, 260, 33, (SPLIT, 2, 1, 4, 0, 2080, 12680), "D = 260: second load of the pair guarded; L = 17: second dalpha block of one wave; A = 33: second tanh slice of one unit"),
    _c("bwd", 2, 33, 516, 8, (SPLIT, 2, 1, 4, 0, 4128, 12808), "D = 516: second trip of the d0 loop; L = 33: second trip of the tanh location loop", dalphas=False),
    _c("bwd", 9, 5, 8, 4, (SPLIT, 8, 2, 4, 0, 256, 38048), "R = 9: passes 8 + 1", dhc_pad=5),
    _c("bwd", 17, 6, 4, 8, (SPLIT, 8, 3, 4, 0, 128, 38080), "R = 17: three passes", dalphas=False),
    # ---- backward, one launch (what D % 4 != 0 or a misaligned ann falls back to)
    _c("bwd", 3, 5, 10, 7, (SINGLE, 3, 1, 1, 0, 4924, 0), "D % 4 != 0: the dalpha kernel's vector loads do not apply", hc_ld=19, dhc_pad=2),
    _c("bwd", 9, 17, 130, 70, (SINGLE, 8, 2, 1, 0, 48088, 0), "lane loop over D three trips, two k0 trips, two passes", dalphas=False),
    _c("bwd", 2, 5, 12, 8, (SINGLE, 2, 1, 1, 0, 5600, 0), "ann 4 bytes past a 16-byte boundary", ann_off=1),
]

CTX_CASES = [
    dict(R=1, L=3, D=1, T1=1, accumulate=0, plan=(13, 13, 208), why="smallest: one location vector, one feature"),
    dict(R=5, L=49, D=256, T1=8, accumulate=1, plan=(13, 13, 8320), why="7x7 map, exactly one block of features, one full trip of 8 steps"),
    dict(R=1, L=52, D=257, T1=9, accumulate=0, plan=(13, 13, 1872), why="L = 52: the last length NQ = 13 takes; second feature block of one thread; 8 + 1 steps"),
    dict(R=5, L=53, D=1, T1=17, accumulate=1, plan=(16, 16, 21760), why="L = 53: first length of NQ = 16, one slab; three step trips"),
    dict(R=5, L=64, D=257, T1=1, accumulate=0, plan=(16, 16, 1280), why="L = 64 fills one slab of 16 exactly"),
    dict(R=1, L=65, D=256, T1=9, accumulate=1, plan=(16, 32, 4608), why="L = 65: two slabs, the second holds one location"),
    dict(R=5, L=196, D=257, T1=8, accumulate=0, plan=(16, 64, 40960), why="14x14 map: four slabs, the last 4 of 16 vectors used"),
]


def step_id(c):
    return "%s-R%d-L%d-D%d-A%d-ld%d%s%s" % (c["op"], c["R"], c["L"], c["D"], c["A"], c["hc_ld"], "" if c["scratch"] else "-noscratch", "-off" if c["ann_off"] else "")


def ctx_id(c):
    return "R%d-L%d-D%d-T%d-acc%d" % (c["R"], c["L"], c["D"], c["T1"], c["accumulate"])


def steps(index):
    """(T1, step): one step alone, or the middle one of three"""
    return (3, 1) if index % 2 else (1, 0)


def lengths_for(R, T1, step):
    """(3 R,) lengths.  Image 1 is dead.  Image 0 alternates live and dead rows in its first pass of 8, is live in a middle pass and dead in
    its last pass when there are several; image 2 is dead in its first pass when there are several, alternates in a middle pass and is live
    in the last (so the last caption row of the batch is live).  R = 1: live, dead, live."""
    live, dead = [step + 1, T1, T1 + 2], [0, step]
    passes = -(-R // 8)
    out = []
    for b in range(B):
        for r in range(R):
            p = r // 8
            if b == 1:
                alive = False
            elif R == 1:
                alive = True
            elif passes == 1:
                alive = (r % 2 == 0) if b == 0 else (r != 0)
            elif b == 0:
                alive = (r % 2 == 0) if p == 0 else p < passes - 1
            else:
                alive = False if p == 0 else (r % 2 == 1) if p < passes - 1 else True
            out.append(live[(b + r) % 3] if alive else dead[r % 2])
    return torch.tensor(out, dtype=torch.int32)


def flags(c, bf16=False):
    return (FLAG_SCRATCH if (c["scratch"] or c["op"] == "bwd") else 0) | (0 if c["ann_off"] else FLAG_ANN_ALIGNED) | FLAG_ROWS_ALIGNED | (FLAG_BF16 if bf16 else 0)


def query(lib, c, T1=1, bf16=False):
    """(status, plan in the layout of the table) of sat_attention_step_plan"""
    import ctypes
    out = (ctypes.c_int32 * 9)()
    if "op" in c:
        rc = lib.sat_attention_step_plan(OPS[c["op"]], B, c["R"], c["L"], c["D"], c["A"], c["hc_ld"], T1, flags(c, bf16), out)
        return rc, (out[0], out[1], out[2], out[3], out[4], out[7], out[8])
    rc = lib.sat_attention_step_plan(OPS["ctx"], B, c["R"], c["L"], c["D"], 0, 0, c["T1"], 0, out)
    return rc, (out[5], out[6], out[7])


def runs_bf16(c):
    """the bf16 annotation stream and the bf16 side outputs exist in the split pair only"""
    return c["plan"][0] == SPLIT


# ------------------------------------------------------------------ inputs
def step_inputs(c, index, dataset="real", bf16=False):
    """Host tensors of one step case (fp32 values; `ann` rounded to bf16 for the bf16 stream).
    real: U, q, dZ, dXZ, dalpha standard normal, ann uniform in (-2, 2), beta a sigmoid of normals, wf standard normal -- and, so that the
    reference alone notices a dropped last location, unit or feature (test_attention_plan.py checks it): the last unit's weight is
    2.5 sqrt(L) (its share of a score is O(1)), the last location's U is c sign(wf) with c such that its tanh terms, all pulling one way, lift its
    score by about 3 (it holds a visible share of every softmax without saturating it) and the last feature's gradients are 8 times the others'.
    int (backward): ann, Z, dZ, dXZ, dalpha integers in -2 .. 2, beta in {0, 1/2, 1}: DZ, the gate gradient and dalpha are exact in fp32
    whatever the order of the additions."""
    R, L, D, A = c["R"], c["L"], c["D"], c["A"]
    N = B * R
    T1, step = steps(index)
    g = torch.Generator().manual_seed(7000 + index)
    nrm = lambda *s: torch.randn(*s, generator=g)
    ints = lambda *s: torch.randint(-2, 3, s, generator=g).float()
    d = dict(T1=T1, step=step, lengths=lengths_for(R, T1, step))
    d["wf"] = nrm(A); d["wf"][A - 1] = 2.5 * L ** 0.5
    d["U"] = nrm(B, L, A)
    pull = min(0.995, 3.0 * L ** 0.5 / float(d["wf"].abs().sum()))          # tanh of the last location's U: about +3 on its score
    d["U"][:, L - 1, :] = float(torch.atanh(torch.tensor(pull))) * torch.sign(d["wf"])
    d["q"] = nrm(N, A)
    if dataset == "int":
        d["ann"], d["beta"] = ints(B, L, D), torch.randint(0, 3, (N, D), generator=g).float() / 2
        d["dZ"], d["dXZ"], d["dalpha"], d["Z_in"] = ints(N, D), ints(N, D), ints(N, L), ints(N, D)
    else:
        d["ann"], d["beta"] = torch.rand(B, L, D, generator=g) * 4 - 2, torch.sigmoid(nrm(N, D))
        d["dZ"], d["dXZ"], d["dalpha"] = nrm(N, D), nrm(N, D), nrm(N, L)
        d["dZ"][:, D - 1] *= 8; d["dXZ"][:, D - 1] *= 8
    if bf16:
        d["ann"] = d["ann"].to(torch.bfloat16).float()
    if not c["dalphas"]:
        d["dalpha"] = None
    return d


def ctx_inputs(c, index, dataset="real"):
    """alphas (N, T1, L), DZ (T1, N, D), lengths holding 0, T1 and T1 + 3 (the last row live), dann0 (B, L, D) to accumulate onto.
    real: alphas a softmax of 2 * normals, DZ and dann0 standard normal.  int: alphas multiples of 1/8 in 0 .. 1, DZ and dann0 integers in
    -2 .. 2: every partial sum is a multiple of 1/8 below 2^10, exact in fp32 in any order."""
    R, L, D, T1 = c["R"], c["L"], c["D"], c["T1"]
    N = B * R
    g = torch.Generator().manual_seed(9000 + index)
    cyc = [T1 + 3, 0, T1, 1, max(T1 - 1, 0)]
    lengths = torch.tensor([cyc[i % 5] for i in range(N)], dtype=torch.int32)
    lengths[N - 1] = T1
    if dataset == "int":
        alphas = torch.randint(0, 9, (N, T1, L), generator=g).float() / 8
        DZ, dann0 = torch.randint(-2, 3, (T1, N, D), generator=g).float(), torch.randint(-2, 3, (B, L, D), generator=g).float()
    else:
        alphas = torch.softmax(2 * torch.randn(N, T1, L, generator=g), dim=2)
        DZ, dann0 = torch.randn(T1, N, D, generator=g), torch.randn(B, L, D, generator=g)
    return dict(alphas=alphas, DZ=DZ, lengths=lengths, dann0=dann0)
