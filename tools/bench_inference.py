"""Dev tool / BASELINE configs[4] (C5): caption() throughput, greedy (beam 1) vs beam 5, resnet50 encoder, 64 images, on one GPU.
Decode-only timing (annotations precomputed) and end-to-end timing (encoder included).
``--topg G`` / ``--prefix-len P`` / ``--no-unk`` time the constrained batched search instead ("Constrained search"): the
prefix of an image is the first P words of its unconstrained caption; the result is checked against the per-image loop.
``--sample-method multinomial|topk|nucleus`` (``--sample-topk``, ``--sample-topp``) times the sampled batched search drawn by the device
generator from a fixed seed: the median of ``--repeats`` timed calls after two warm-up calls.
``--no-repeat-ngram N`` / ``--min-length M`` / ``--repetition-penalty X`` time the batched search under the history rules (DESIGN.md 5,
"History rules") next to the plain batched search, alternating the two over ``--repeats`` calls each; ``--skip-loop`` leaves the
per-image loop (the slowest line, and the check of the result) out.
``--beam-groups G [G ...]`` / ``--diversity-penalty X`` time the diverse beam search ("Diverse beam search") next to the plain
batched search at the same beam, alternating over ``--repeats`` calls each (every G must divide the beam); the lines report distinct-1 /
distinct-2 of the images' full beams (``metrics.distinct_n``, means over the 64 images) and the selection kernel's own time, taken with
events around ``sat_beam_group_select`` on scores of the search's shape, times the steps of the search.
``--ensemble M [M ...]`` / ``--ensemble-combine arithmetic|geometric`` time ensemble decoding ("Ensemble decoding") over M
differently seeded bench models, each on its own encoder's annotations, next to the plain batched search of the first model, alternating
over ``--repeats`` calls each; the lines report the ratio to M plain searches and the combine kernel's own time and bandwidth, taken with
events around ``sat_beam_ensemble_scores`` on logits of the search's shape, times the steps of the search.
``--required C [C ...]`` times the search with required words ("Required words") next to the plain batched search at the same
beam, alternating over ``--repeats`` calls each: every image gets C distinct random non-special ids from a fixed seed.  The lines report the
ratio to the plain line, the coverage (``constraints.required_coverage``, mean over the 64 images) of the plain and of the required
search's captions, and the selection kernel's own time next to the block top-k of ``beam_select_kernel`` on the same scores, each taken
with events around 21 launches."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import sat_amd  # noqa
from sat_amd import model as M

ap = argparse.ArgumentParser()
ap.add_argument("precision", nargs="?", default="bf16", choices=["bf16", "fp32"])
ap.add_argument("--topg", type=int, default=None)
ap.add_argument("--prefix-len", type=int, default=0)
ap.add_argument("--no-unk", action="store_true")
ap.add_argument("--beams", type=int, nargs="+", default=[1, 5])
ap.add_argument("--sample-method", default="beam", choices=["beam", "multinomial", "topk", "nucleus"])
ap.add_argument("--sample-topk", type=int, default=3)
ap.add_argument("--sample-topp", type=float, default=0.9)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--no-repeat-ngram", type=int, default=None, help="no n-gram of this size is said twice in a caption (0 / unset = off)")
ap.add_argument("--min-length", type=int, default=None, help="<END> stays masked until a caption has this many words")
ap.add_argument("--repetition-penalty", type=float, default=None, help="CTRL's penalty on the logits of the words already said (1.0 = off)")
ap.add_argument("--skip-loop", action="store_true")
ap.add_argument("--beam-groups", type=int, nargs="+", default=None, help="groups of the diverse beam search, each a divisor of every beam (1 = the plain search)")
ap.add_argument("--diversity-penalty", type=float, default=0.5, help="what a group pays per hypothesis an earlier group kept with the same word at a step")
ap.add_argument("--ensemble", type=int, nargs="+", default=None, help="member counts of the ensemble search (1 = one model, which delegates to the plain search)")
ap.add_argument("--ensemble-combine", default="arithmetic", choices=["arithmetic", "geometric"])
ap.add_argument("--required", type=int, nargs="+", default=None, help="required words per image: distinct random non-special ids, fixed seed")
a = ap.parse_args()
constrained = a.topg is not None or a.prefix_len > 0 or a.no_unk
history = dict(no_repeat_ngram=a.no_repeat_ngram, min_length=a.min_length, repetition_penalty=a.repetition_penalty)
history_on = any(v is not None for v in history.values())



def select_kernel_ms(beamk, groups, V, steps, lam):
    """beam_group_select_kernel alone: ``steps`` launches on (64, beamk, V) scores between two events, every group full"""
    from sat_amd import _lib as L
    sc = torch.randn(64, beamk, V, device="cuda")
    kl = torch.full((64, groups), beamk // groups, dtype=torch.int32, device="cuda")
    work, vals, inds = torch.empty_like(sc), torch.empty(64, beamk, device="cuda"), torch.empty(64, beamk, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for rep in range(5):
        e0.record()
        for _ in range(steps):
            L.check(L.lib().sat_beam_group_select(L.ptr(sc), L.ptr(kl), 64, beamk, groups, V, 0, lam, L.ptr(work), L.ptr(vals), L.ptr(inds), L.stream_ptr()),
                    "sat_beam_group_select")
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out[1:])


def required_words(n_images, count, V, special, seed=1234):
    """``count`` distinct non-special ids per image from a fixed seed"""
    g = torch.Generator().manual_seed(seed + count)
    ok = torch.tensor([t for t in range(V) if t not in special])
    return [ok[torch.randperm(len(ok), generator=g)[:count]].tolist() for _ in range(n_images)]


def required_kernel_ms(beamk, V, steps, words, end_id):
    """(beam_required_select_kernel with the words, and without any: the block top-k that beam_select_kernel runs at a free step) alone:
    ``steps`` launches each on the same (64, beamk, V) scores between two events, every row live; the rows have said ``steps // 2`` random
    words and, every second row, the image's first required word"""
    import ctypes as C
    from sat_amd import _lib as L
    lib = L.lib()
    n = len(words)
    sc = torch.randn(n, beamk, V, device="cuda")
    kl = torch.full((n,), beamk, dtype=torch.int32, device="cuda")
    stride, said = steps, steps // 2
    hist = torch.randint(0, V, (n * beamk, stride), dtype=torch.int32, device="cuda")
    wd = torch.tensor(words, dtype=torch.int32, device="cuda")
    hist.view(n, beamk, stride)[:, ::2, 0] = wd[:, :1]
    nw = torch.full((n,), wd.shape[1], dtype=torch.int32, device="cuda")
    req = L.BeamRequired(max_required=wd.shape[1], words=wd.data_ptr(), n_words=nw.data_ptr())
    off = L.BeamRequired(max_required=0)
    work, vals, inds = torch.empty_like(sc), torch.empty(n, beamk, device="cuda"), torch.empty(n, beamk, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def required():
        L.check(lib.sat_beam_required_select(L.ptr(sc), L.ptr(kl), n, beamk, V, L.ptr(hist), stride, said, 0, C.byref(req), end_id, L.ptr(work), L.ptr(vals),
                                             L.ptr(inds), L.stream_ptr()), "sat_beam_required_select")

    def plain():                                            # no words: beam_block_topk over the k * V scores, beam_select_kernel's free step
        L.check(lib.sat_beam_required_select(L.ptr(sc), L.ptr(kl), n, beamk, V, L.ptr(hist), stride, said, 0, C.byref(off), end_id, L.ptr(work), L.ptr(vals),
                                             L.ptr(inds), L.stream_ptr()), "sat_beam_required_select")
    out = []
    for launch in (required, plain):
        times = []
        for rep in range(5):
            e0.record()
            for _ in range(steps):
                launch()
            e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        out.append(statistics.median(times[1:]))
    return out


def combine_kernel_ms(members, rows, V, steps, combine):
    """beam_ensemble_combine_kernel alone: ``steps`` launches on ``members`` x (rows, V) logits between two events"""
    import ctypes as C
    from sat_amd import _lib as L
    zs = [torch.randn(rows, V, device="cuda") for _ in range(members)]
    out = torch.empty(rows, V, device="cuda")
    arr = (C.c_void_p * members)(*[z.data_ptr() for z in zs]); wts = (C.c_float * members)(*([1.0 / members] * members))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for rep in range(5):
        e0.record()
        for _ in range(steps):
            L.check(L.lib().sat_beam_ensemble_scores(arr, wts, members, L.ENSEMBLE_COMBINE[combine], rows, V, 1.0, L.ptr(out), L.stream_ptr()),
                    "sat_beam_ensemble_scores")
        e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times[1:])


hp, T, B, R = bench.hparams("c2")
torch.manual_seed(42)
model = M.SAT(**hp).cuda().eval(); model.set_precision(a.precision)
img = torch.rand(64, 3, hp["input_size"], hp["input_size"], device="cuda")
with torch.no_grad():
    ann, hw = model.encode(img)
    ann = ann.contiguous()
    members = []
    if a.ensemble:
        from sat_amd.ensemble import Ensemble
        members = [(model, ann)]
        for i in range(1, max(a.ensemble)):
            torch.manual_seed(42 + i)
            other = M.SAT(**hp).cuda().eval(); other.set_precision(a.precision)
            members.append((other, other.encode(img)[0].contiguous()))
    for beamk in a.beams:
        if a.ensemble:
            settings = [("plain", model, ann)]
            settings += [("M=%d" % m, Ensemble([x[0] for x in members[:m]], combine=a.ensemble_combine), [x[1] for x in members[:m]]) for m in a.ensemble]
            times, caps = {name: [] for name, _, _ in settings}, {}
            for name, mod, anns in settings:
                for _ in range(2):
                    caps[name] = mod.beam_decode_batched(anns, hw, beamk=beamk, max_gen_length=20)[0]
            for _ in range(a.repeats):                  # alternate, so that every line sees the same machine
                for name, mod, anns in settings:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    mod.beam_decode_batched(anns, hw, beamk=beamk, max_gen_length=20)
                    torch.cuda.synchronize(); times[name].append(time.perf_counter() - t0)
            mp = statistics.median(times["plain"])
            for (name, _, _), m in zip(settings, [0] + list(a.ensemble)):
                t = times[name]
                extra = ""
                if m >= 1:
                    rows, V = 64 * beamk, hp["vocab_size"]
                    ms = combine_kernel_ms(m, rows, V, 21, a.ensemble_combine)
                    extra = (", %.3fx of %d plain searches, %d of 64 captions differ from the first model's, combine kernel alone %.3f ms for 21 steps "
                             "(%.0f GB/s of (M + 1) N V 4 bytes)" % (statistics.median(t) / (m * mp), m, sum(x != y for x, y in zip(caps[name], caps["plain"])), ms,
                                                                  21 * (m + 1) * rows * V * 4 / (ms * 1e-3) / 1e9))
                print("beam %d %s (%s): median %.2f ms (min %.2f, max %.2f) per 64 images incl. host back-trace over %d calls%s"
                      % (beamk, name, a.ensemble_combine, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, a.repeats, extra))
            continue
        if a.required:
            from sat_amd.constraints import required_coverage
            special = {int(hp["vocab_stoi"][s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")}
            words = {c: required_words(64, c, hp["vocab_size"], special) for c in a.required}
            settings = [("plain", dict(beamk=beamk, max_gen_length=20))]
            settings += [("C=%d" % c, dict(beamk=beamk, max_gen_length=20, required=words[c])) for c in a.required]
            times, caps = {name: [] for name, _ in settings}, {}
            for name, kw in settings:
                for _ in range(2):
                    caps[name] = model.beam_decode_batched(ann, hw, **kw)[0]
            for _ in range(a.repeats):                  # alternate, so that every line sees the same machine
                for name, kw in settings:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    model.beam_decode_batched(ann, hw, **kw)
                    torch.cuda.synchronize(); times[name].append(time.perf_counter() - t0)
            mp = statistics.median(times["plain"])
            for (name, kw), c in zip(settings, [0] + list(a.required)):
                t = times[name]
                extra = ""
                if c:
                    ms_req, ms_plain = required_kernel_ms(beamk, hp["vocab_size"], 21, words[c], int(hp["vocab_stoi"]["<END>"]))
                    extra = (", %.3fx the plain line, coverage %.3f (the plain search's captions: %.3f), selection kernel alone %.2f ms for 21 steps "
                             "(beam_select_kernel's block top-k on the same scores: %.2f ms)"
                             % (statistics.median(t) / mp, sum(required_coverage(caps[name], words[c])) / 64,
                                sum(required_coverage(caps["plain"], words[c])) / 64, ms_req, ms_plain))
                print("beam %d %s: median %.2f ms (min %.2f, max %.2f) per 64 images incl. host back-trace over %d calls%s"
                      % (beamk, name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, a.repeats, extra))
            continue
        if a.beam_groups:
            from sat_amd.metrics import distinct_n
            settings = [("plain", dict(beamk=beamk, max_gen_length=20))]
            settings += [("G=%d" % g, dict(beamk=beamk, max_gen_length=20, beam_groups=g, diversity_penalty=a.diversity_penalty)) for g in a.beam_groups]
            times, div = {name: [] for name, _ in settings}, {}
            for name, kw in settings:
                for _ in range(2):
                    every = model.beam_decode_batched(ann, hw, return_all=True, **kw)[0]
                div[name] = [sum(distinct_n(caps, n) for caps in every) / 64 for n in (1, 2)]
            for _ in range(a.repeats):                  # alternate, so that every line sees the same machine
                for name, kw in settings:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    model.beam_decode_batched(ann, hw, **kw)
                    torch.cuda.synchronize(); times[name].append(time.perf_counter() - t0)
            mp = statistics.median(times["plain"])
            for name, kw in settings:
                t = times[name]
                extra = ""
                if name != "plain":
                    extra = ", %.3fx the plain line, selection kernel alone %.2f ms for 21 steps" % (
                        statistics.median(t) / mp, select_kernel_ms(beamk, kw["beam_groups"], hp["vocab_size"], 21, a.diversity_penalty))
                print("beam %d %s (diversity_penalty=%g): median %.2f ms (min %.2f, max %.2f) per 64 images incl. host back-trace over %d calls, "
                      "distinct-1 %.3f distinct-2 %.3f%s" % (beamk, name, a.diversity_penalty, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                              a.repeats, div[name][0], div[name][1], extra))
            continue
        if history_on:
            plain_kw = dict(beamk=beamk, max_gen_length=20)
            rule_kw = dict(plain_kw, sample_method=a.sample_method, sample_topk=a.sample_topk, sample_topp=a.sample_topp, topg=a.topg, no_unk=a.no_unk, **history)
            if a.sample_method != "beam":
                rule_kw["seed"] = 7
            for _ in range(2):
                caps = model.beam_decode_batched(ann, hw, **plain_kw)[0]
                capsh = model.beam_decode_batched(ann, hw, **rule_kw)[0]
            if not a.skip_loop and a.sample_method == "beam":
                capsl = model.beam_decode(ann, hw, **rule_kw)[0]
                print("beam %d: %d of 64 captions under the rules equal the per-image loop's" % (beamk, sum(x == y for x, y in zip(capsh, capsl))))
            tp, th = [], []
            for _ in range(a.repeats):                  # alternate, so that both lines see the same machine
                for kw, times in ((plain_kw, tp), (rule_kw, th)):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    model.beam_decode_batched(ann, hw, **kw)
                    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
            mp, mh = statistics.median(tp), statistics.median(th)
            print("beam %d: batched search, rules off: median %.2f ms (min %.2f, max %.2f) per 64 images incl. host back-trace over %d calls"
                  % (beamk, mp * 1e3, min(tp) * 1e3, max(tp) * 1e3, a.repeats))
            print("beam %d: batched search, history rules (no_repeat_ngram=%s, min_length=%s, repetition_penalty=%s, %s): median %.2f ms (min %.2f, max %.2f), "
                  "%.3fx the rules-off line, %d of 64 captions differ, mean caption length %.1f"
                  % (beamk, a.no_repeat_ngram, a.min_length, a.repetition_penalty, a.sample_method, mh * 1e3, min(th) * 1e3, max(th) * 1e3, mh / mp,
                     sum(x != y for x, y in zip(capsh, caps)), sum(len(c) + 1 for c in capsh) / 64))
            continue
        for _ in range(2):
            model.beam_decode(ann[:8], hw, beamk=beamk, max_gen_length=20)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        caps, scores, alphas, ppl = model.beam_decode(ann, hw, beamk=beamk, max_gen_length=20)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        steps = sum(len(c) + 1 for c in caps)
        print("beam %d: decode-only %.1f images/s (%.1f ms/image, mean caption length %.1f, %.0f us per decode step of the kept hypothesis)"
              % (beamk, 64 / dt, dt / 64 * 1e3, steps / 64, dt / steps * 1e6))
        if constrained:
            special = {int(hp["vocab_stoi"][s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")}
            prefix = [c[:min([a.prefix_len] + [i for i, t in enumerate(c) if t in special])] for c in caps]
            kw = dict(beamk=beamk, max_gen_length=20, topg=a.topg, prefix=prefix if a.prefix_len > 0 else None, no_unk=a.no_unk)
            capsl = model.beam_decode(ann, hw, **kw)[0]
            for _ in range(2):
                model.beam_decode_batched(ann, hw, **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(5):
                capsc, _, _, _ = model.beam_decode_batched(ann, hw, **kw)
            torch.cuda.synchronize(); dtc = (time.perf_counter() - t0) / 5
            assert capsc == capsl
            print("beam %d: constrained batched search (topg=%s, prefix-len=%d, no-unk=%s), decode-only %.0f images/s (%.2f ms per 64 images incl. host "
                  "back-trace), %d of 64 captions differ from the unconstrained search"
                  % (beamk, a.topg, a.prefix_len, a.no_unk, 64 / dtc, dtc * 1e3, sum(x != y for x, y in zip(capsc, caps))))
            continue
        if a.sample_method != "beam":
            kw = dict(beamk=beamk, max_gen_length=20, sample_method=a.sample_method, sample_topk=a.sample_topk, sample_topp=a.sample_topp, seed=7)
            for _ in range(2):
                model.beam_decode_batched(ann, hw, **kw)
            times = []
            for _ in range(a.repeats):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                capss = model.beam_decode_batched(ann, hw, **kw)[0]
                torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
            dts = statistics.median(times)
            print("beam %d: sampled batched search (%s, sample_topk=%d, sample_topp=%g), decode-only %.0f images/s (median %.2f ms, min %.2f, max %.2f per 64 images "
                  "incl. host back-trace over %d calls), mean caption length %.1f"
                  % (beamk, a.sample_method, a.sample_topk, a.sample_topp, 64 / dts, dts * 1e3, min(times) * 1e3, max(times) * 1e3, a.repeats,
                     sum(len(c) + 1 for c in capss) / 64))
            continue
        for _ in range(2):
            model.beam_decode_batched(ann, hw, beamk=beamk, max_gen_length=20)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5):
            capsb, _, _, _ = model.beam_decode_batched(ann, hw, beamk=beamk, max_gen_length=20)
        torch.cuda.synchronize(); dtb = (time.perf_counter() - t0) / 5
        assert capsb == caps
        print("beam %d: batched search, decode-only %.0f images/s (%.2f ms per 64 images incl. host back-trace), %.1fx the per-image loop"
              % (beamk, 64 / dtb, dtb * 1e3, dt / dtb))
        for _ in range(2):
            model.beam_decode_batched(ann, hw, beamk=beamk, max_gen_length=20, graph=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5):
            capsg, _, _, _ = model.beam_decode_batched(ann, hw, beamk=beamk, max_gen_length=20, graph=True)
        torch.cuda.synchronize(); dtg = (time.perf_counter() - t0) / 5
        assert capsg == caps
        print("beam %d: batched search replayed from a hipGraph, decode-only %.0f images/s (%.2f ms per 64 images incl. host back-trace)" % (beamk, 64 / dtg, dtg * 1e3))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            model.caption(img, beamk=beamk, max_gen_length=20)
        torch.cuda.synchronize(); dte = (time.perf_counter() - t0) / 3
        print("beam %d: caption() end to end (encoder + batched decode) %.0f images/s" % (beamk, 64 / dte))
