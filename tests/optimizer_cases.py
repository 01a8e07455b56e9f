"""The launches that pin every form of the fused optimizer step (csrc/optimizer.hip), and, mirrored in Python, the predicates by which
the kernels choose a form.  test_optimizer_cases.py (no GPU) asserts that the table reaches every form; test_gpu_optimizer_forms.py
runs it.  When a predicate in the kernels changes, the mirror here changes with it and the table is re-derived until it reaches every
form again: a form that is no longer reached fails, nothing thins out silently.

The kernels (one workgroup of 256 lanes per chunk row, `chunks[blockIdx.x]`):
    STEP   optimizer_step_kernel       sat_optimizer_step / _dev           streams p g m v            + the bf16 copy of p
    AVG    optimizer_step_avg_kernel   sat_optimizer_step_avg / _avg_dev   streams p g m v a          + the bf16 copy
    SWAP   optimizer_swap_kernel       sat_optimizer_swap                  streams p a                + the bf16 copy
    NORM   grad_sqsum_part_kernel + grad_norm_finish_kernel   sat_grad_clip_coef   stream g, scalar loads only

Width.  A chunk takes the wide path (float4 loads / stores, one 4 x bf16 store) when every stream the kernel touches starts on a 16-byte
boundary and the bf16 copy on an 8-byte one (NULL counts as aligned).  STEP looks at p, g, m, v whether or not the kind reads them; AVG
looks at m and v only when the kind reads them (not ASGD, not NULL) and at the average also when it is NULL (0); SWAP looks at p and a.
Otherwise every element goes through the 4-byte loop (2-byte stores of the copy).

Extent.  A chunk row (tensor, start) covers len = min(65536, n - start) elements.  Wide: nv = len // 4 vectors, lane q takes vectors
q, q + 256, ..., then a tail of len - 4 nv < 4 elements on lanes 0..2.  Narrow: lane q takes elements q, q + 256, ....
"""
import itertools

CHUNK = 65536
STEP, AVG, SWAP, NORM = "step", "step_avg", "swap", "clip_coef"
STREAMS = {STEP: ("p", "g", "m", "v"), AVG: ("p", "g", "m", "v", "a"), SWAP: ("p", "a"), NORM: ("g",)}
ENTRIES = {STEP: ("sat_optimizer_step", "sat_optimizer_step_dev"), AVG: ("sat_optimizer_step_avg", "sat_optimizer_step_avg_dev"),
           SWAP: ("sat_optimizer_swap",), NORM: ("sat_grad_clip_coef",)}
SGD, ADAM, ADAMW, ASGD = 0, 1, 2, 3

#: kind name -> (SAT_OPT_*, fields of sat_opt_hyper).  The betas are at least 0.5; bias corrections as after step 3.
KINDS = {
    "sgd": (SGD, dict()),                                                      # no momentum: m is NULL (or, when given, read and written back)
    "sgd_first": (SGD, dict(momentum=0.9, first_step=1)),                      # momentum buffer = gradient
    "sgd_nesterov": (SGD, dict(momentum=0.9, nesterov=1, first_step=0)),
    "adam": (ADAM, dict(beta1=0.8, beta2=0.95, eps=1e-8, bias_correction1=1 - 0.8 ** 3, bias_correction2_sqrt=(1 - 0.95 ** 3) ** 0.5)),
    "adamw": (ADAMW, dict(beta1=0.9, beta2=0.999, eps=1e-8, bias_correction1=1 - 0.9 ** 3, bias_correction2_sqrt=(1 - 0.999 ** 3) ** 0.5)),
    "asgd": (ASGD, dict()),
}
LAMBD = 1e-2          # of every ASGD case


def reads(kernel, kind):
    """the streams a kind reads (and writes back) beside p and g"""
    code = KINDS[kind][0]
    if kernel in (SWAP, NORM):
        return ()
    if code == ASGD:
        return ()
    if code == SGD:
        return ("m",) if KINDS[kind][1].get("momentum", 0.0) != 0 else ()
    return ("m", "v")


def tensor(n, lr=1e-2, wd=0.0, mis=None, shadow=None, m=True, avg=True, omit=False):
    """one row of the tensor table.  mis: the one stream that starts one float off a 16-byte boundary (None: all aligned); shadow: None
    (no bf16 copy) or its start's offset in bytes from a 16-byte boundary (0, 2, 8); m: False passes m = NULL; avg: False puts NULL into
    the average table; omit: no chunk row names this tensor"""
    assert mis in (None, "p", "g", "m", "v", "a") and shadow in (None, 0, 2, 8)
    return dict(n=n, lr=lr, wd=wd, mis=mis, shadow=shadow, m=m, avg=avg, omit=omit)


def offsets(kernel, kind, t):
    """byte offset mod 16 of every stream the launch passes for this tensor; None = NULL.  (The test asserts data_ptr() % 16 against it.)
    p and g always; m unless the row says m = NULL; v for Adam / AdamW, for ASGD (which must not touch it) and, with m, for SGD (which
    hands it through); the average unless the row's entry is NULL"""
    off = {s: (4 if t["mis"] == s else 0) for s in STREAMS[kernel]}
    if kernel in (STEP, AVG):
        assert t["m"] or KINDS[kind][0] == SGD
        if not t["m"]:
            off["m"] = off["v"] = None
    if "a" in off and not t["avg"]:
        off["a"] = None
    off["shadow"] = t["shadow"]
    return off


def is_wide(kernel, kind, off):
    """the kernels' `vec` predicate on the offsets of offsets()"""
    def a16(s):
        return off.get(s) is None or off[s] % 16 == 0
    if kernel == NORM:
        return False
    sh8 = off["shadow"] is None or off["shadow"] % 8 == 0
    if kernel == STEP:
        return a16("p") and a16("g") and a16("m") and a16("v") and sh8
    if kernel == AVG:
        mv = KINDS[kind][0] != ASGD          # has_m / has_v: not ASGD and not NULL
        return a16("p") and a16("g") and (not mv or (a16("m") and a16("v"))) and a16("a") and sh8
    return a16("p") and a16("a") and sh8


def chunk_rows(tensors):
    """the chunk table as optim.py builds it: (tensor, start) per 65536 elements, tensors in order, omitted ones left out"""
    return [(ti, s) for ti, t in enumerate(tensors) if not t["omit"] for s in range(0, t["n"], CHUNK)]


def n_chunks(n):
    return -(-n // CHUNK)


def extent(n, start, wide):
    """(len, nv, tail, trips of the busiest lane in the body, trips in the tail loop)"""
    ln = min(CHUNK, n - start)
    if wide:
        nv = ln // 4
        return ln, nv, ln - 4 * nv, -(-nv // 256), 1 if ln % 4 else 0
    return ln, 0, ln, 0, -(-ln // 256)


def case(name, kernel, kind, tensors, why, clip_coef=None, clip_value=0.0, avg_coef=None, shuffle=False, exact=False):
    """clip_coef: None = NULL pointer, else the value of clip_coef[0]; avg_coef: sat_opt_avg_hyper.coef (AVG only); shuffle: the chunk rows
    in a shuffled order; exact: p must equal the once-rounded reference bit for bit (plain SGD, lr a power of two)"""
    assert (avg_coef is not None) == (kernel == AVG)
    assert kernel in (AVG,) or KINDS[kind][0] != ASGD
    return dict(name=name, kernel=kernel, kind=kind, tensors=tensors, why=why, clip_coef=clip_coef, clip_value=clip_value, avg_coef=avg_coef,
                shuffle=shuffle, exact=exact)


EXTENTS = (1, 3, 4, 5, 1023, 1025, 65535, 65536, 65537, 131072 + 3)
NARROW_EXTENTS = (5, 65537, 131072 + 3)


def _extent_tensors(shadow_every=3):
    """every extent, wide, with three learning rates / weight decays; every third tensor keeps a 16-byte aligned bf16 copy"""
    rates = [(1e-2, 0.0), (3e-3, 0.05), (1e-3, 0.0)]
    return [tensor(n, *rates[i % 3], shadow=0 if i % shadow_every == 0 else None) for i, n in enumerate(EXTENTS)]


def _narrow_tensors(stream, shadow=None):
    """the narrow extents with `stream` one float off, beside one aligned tensor (a launch mixes both paths)"""
    return [tensor(n, 3e-3, 0.05, mis=stream, shadow=shadow) for n in NARROW_EXTENTS] + [tensor(1025, 1e-2, 0.0, shadow=0)]


CASES = []
# ---- every extent on the wide path, every kind, in both step kernels
for _kernel, _kinds in ((STEP, ("sgd", "sgd_first", "sgd_nesterov", "adam", "adamw")), (AVG, ("sgd", "sgd_first", "sgd_nesterov", "adam", "adamw", "asgd"))):
    for _i, _kind in enumerate(_kinds):
        _ts = _extent_tensors()
        if _kind == "sgd":
            for _t in _ts[::2]:
                _t["m"] = False          # m = NULL on half of the tensors, a buffer that must come back untouched on the others
        if _kernel == AVG:
            _ts[1]["avg"] = False; _ts[8]["avg"] = False          # NULL entries in the average table beside non-NULL ones
        _ts[4]["omit"] = _kind in ("adam", "asgd")               # a chunk table that leaves one tensor out
        CASES.append(case("%s-%s-extents" % (_kernel, _kind), _kernel, _kind, _ts, "every extent, wide, three lr / wd groups in one launch",
                          clip_coef=(None, 0.37, 1.0)[_i % 3], clip_value=(0.0, 0.4)[_i % 2],
                          avg_coef=None if _kernel == STEP else (0.1, 1.0, 0.0, 0.25, 1.0, 0.5)[_i], shuffle=bool(_i % 2)))
# ---- the narrow path, forced by each stream alone, across chunk boundaries
for _kernel in (STEP, AVG):
    for _i, _s in enumerate(STREAMS[_kernel]):
        CASES.append(case("%s-adam-narrow-%s" % (_kernel, _s), _kernel, "adam", _narrow_tensors(_s, shadow=(None, 0)[_i % 2]),
                          "%s alone is one float off 16 bytes" % _s, clip_coef=(0.37, None)[_i % 2], clip_value=(0.4, 0.0)[_i % 2],
                          avg_coef=None if _kernel == STEP else (0.1, 0.0, 1.0, 0.25, 0.5)[_i], shuffle=bool(_i % 2)))
CASES += [
    case("step-sgd-narrow-m", STEP, "sgd", _narrow_tensors("m"), "the plain kernel looks at m although the kind does not use it: narrow"),
    case("step_avg-sgd-narrow-m", AVG, "sgd", _narrow_tensors("m"), "so does the averaging kernel for a buffer that is not NULL", avg_coef=0.1),
    case("step_avg-asgd-m-off-stays-wide", AVG, "asgd", _narrow_tensors("m"), "ASGD never touches m and v: their alignment does not matter, wide", avg_coef=0.1),
    case("step_avg-asgd-narrow-p", AVG, "asgd", _narrow_tensors("p", shadow=0), "ASGD on the narrow path", clip_value=0.4, avg_coef=0.25, shuffle=True),
    case("step_avg-asgd-narrow-a", AVG, "asgd", _narrow_tensors("a"), "ASGD, the average one float off", clip_coef=0.37, avg_coef=1.0),
    case("step-sgd_nesterov-narrow-g", STEP, "sgd_nesterov", _narrow_tensors("g", shadow=0), "SGD with momentum on the narrow path", clip_coef=0.37),
]
# ---- the bf16 copy: 2-byte aligned -> narrow, 8 but not 16 -> still wide, in all three writing kernels
for _kernel, _kind in ((STEP, "adam"), (AVG, "adamw"), (SWAP, "sgd")):
    _kw = dict(avg_coef=0.1) if _kernel == AVG else {}
    CASES.append(case("%s-copy-2-bytes" % _kernel, _kernel, _kind, [tensor(n, 3e-3, 0.05, shadow=2) for n in NARROW_EXTENTS] + [tensor(1025, shadow=0)],
                      "the bf16 copy one element off: 2-byte stores only", **_kw))
    CASES.append(case("%s-copy-8-bytes" % _kernel, _kernel, _kind, [tensor(n, 3e-3, 0.05, shadow=8) for n in (5, 1023, 65537, 131072 + 3)],
                      "the bf16 copy 8 but not 16 bytes aligned: the 8-byte store is still aligned, wide", **_kw))
# ---- the swap kernel
CASES += [
    case("swap-extents", SWAP, "sgd", [dict(t, avg=i not in (1, 8), omit=i == 4) for i, t in enumerate(_extent_tensors(2))],
         "every extent, wide; two tensors without an average, one left out of the chunk table", shuffle=True),
    case("swap-narrow-p", SWAP, "sgd", _narrow_tensors("p", shadow=0), "p one float off"),
    case("swap-narrow-a", SWAP, "sgd", _narrow_tensors("a", shadow=0), "the average one float off", shuffle=True),
]
# ---- bit-exact outputs
CASES.append(case("step-sgd-exact", STEP, "sgd", [tensor(n, 2.0 ** -6, 0.0, m=False, shadow=0) for n in (5, 1025, 65537)],
                  "plain SGD, lr a power of two: lr g is exact, p - lr g rounds once", exact=True))
CASES.append(case("step_avg-sgd-exact", AVG, "sgd", [tensor(n, 2.0 ** -6, 0.0, m=False, mis=mis) for n, mis in ((5, None), (1025, "g"), (65537, None))],
                  "the same through the averaging kernel, coefficient 1: a == p", avg_coef=1.0, exact=True))

#: sat_grad_clip_coef: (name, sizes, index of the tensor whose g is one float off, fill) - ragged last chunks, several tensors
NORM_CASES = [
    ("ragged", (5, 65537, 131072 + 3, 1023, 1), 2, "randn"),
    ("zeros", (5, 65537, 1023), 1, "zeros"),
    ("1e20", (5, 65537, 1023), 1, "1e20"),
    ("nan", (5, 65537, 131072 + 3, 1023), 2, "nan"),
    ("inf", (5, 65537, 1023), 1, "inf"),
]


def forms_reached():
    """what the table reaches, read off the table through the mirrored predicates"""
    seen = set()
    for c in CASES:
        kernel, kind = c["kernel"], c["kind"]
        for e in ENTRIES[kernel]:
            seen.add(("entry", e))
        seen.add(("kind", kernel, kind))
        seen.add(("clip_coef", kernel, "NULL" if c["clip_coef"] is None else "set"))
        seen.add(("clip_value", kernel, "0" if c["clip_value"] == 0 else ">0"))
        if c["avg_coef"] is not None:
            seen.add(("avg coef", "0" if c["avg_coef"] == 0 else "1" if c["avg_coef"] == 1 else "between", "asgd" if kind == "asgd" else "ema"))
        if c["shuffle"]:
            seen.add(("shuffled rows", kernel))
        if len({(t["lr"], t["wd"]) for t in c["tensors"]}) > 1:
            seen.add(("several lr / wd", kernel))
        if kernel == AVG and {t["avg"] for t in c["tensors"] if not t["omit"]} == {True, False}:
            seen.add(("NULL beside non-NULL averages", kernel))
        if kernel == SWAP and {t["avg"] for t in c["tensors"] if not t["omit"]} == {True, False}:
            seen.add(("NULL beside non-NULL averages", kernel))
        widths = set()
        for t in c["tensors"]:
            off = offsets(kernel, kind, t)
            wide = is_wide(kernel, kind, off)
            if t["omit"]:
                seen.add(("omitted tensor", kernel))
                continue
            widths.add(wide)
            if kernel != SWAP and t["wd"] != 0:
                seen.add(("weight decay", kernel, kind))
            if kernel != SWAP and off.get("m") is None and KINDS[kind][0] == SGD:
                seen.add(("m NULL", kernel))
            mis = [s for s in STREAMS[kernel] if off.get(s) == 4]
            assert len(mis) <= 1
            if mis:
                seen.add(("one float off", kernel, mis[0], "wide" if wide else "narrow"))
            if off["shadow"] is not None:
                seen.add(("copy", kernel, off["shadow"], "wide" if wide else "narrow"))
            for start in range(0, t["n"], CHUNK):
                ln, nv, tail, body, tails = extent(t["n"], start, wide)
                if wide:
                    seen.add(("wide", kernel, "n", t["n"]))
                    seen.add(("wide", kernel, "tail", tail))
                    seen.add(("wide", kernel, "body trips", min(body, 2)))
                    if off["shadow"] is not None:
                        seen.add(("copy written by", kernel, "body" if nv else None))
                        seen.add(("copy written by", kernel, "tail" if tail else None))
                else:
                    seen.add(("narrow", kernel, "n", t["n"]))
                    if start > 0:
                        seen.add(("narrow", kernel, "chunk start > 0", "full" if ln == CHUNK else "ragged"))
                    if off["shadow"] is not None:
                        seen.add(("copy written by", kernel, "narrow"))
        if widths == {True, False}:
            seen.add(("both paths in one launch", kernel))
    for name, sizes, mis, fill in NORM_CASES:
        seen.add(("entry", ENTRIES[NORM][0]))
        seen.add(("norm", fill))
        if len(sizes) > 1 and any(n % CHUNK for n in sizes):
            seen.add(("norm", "ragged last chunks"))
        if mis is not None:
            seen.add(("norm", "misaligned g"))
    return seen


def all_tensor_sizes():
    return sorted({t["n"] for c in CASES for t in c["tensors"]} | {n for _, sizes, _, _ in NORM_CASES for n in sizes})


def sweep():
    """(n, start) of every chunk row of every size within a few elements of the edges: for the arithmetic checks of the CPU test"""
    ns = set(itertools.chain.from_iterable((e - 1, e, e + 1) for e in (1, 4, 1024, CHUNK, 2 * CHUNK, 2 * CHUNK + 4))) - {0}
    return [(n, s) for n in sorted(ns | set(EXTENTS)) for s in range(0, n, CHUNK)]
