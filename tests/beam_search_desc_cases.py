"""One batched search through an entry point from before the descriptor and through sat_beam_search (include/sat_hip.h), from the same
parts: what tests/test_beam_search_desc.py (host pointers, refusals only) and tests/test_gpu_beam_search_desc.py (device buffers) share."""
import ctypes as C

OUTPUTS = ("tok_in", "prev_row", "alpha_hist", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean")
ENTRIES = ("batched", "sampled", "constrained", "history", "groups", "required", "ensemble")


class Parts:
    """what a search is asked to do: a single model (dims, w, ann) or an ensemble, sizes, host arrays and the feature structs (None = off)"""

    def __init__(self, dims=None, w=None, ann=None, ens=None, beamk=4, S=6, temps=(1.0,), ids=(0, 1, 2, 3), smp=None, con=None, hist=None, grp=None,
                 req=None, keep=None):
        self.dims, self.w, self.ann, self.ens, self.beamk, self.S = dims, w, ann, ens, beamk, S
        self.temps = (C.c_float * len(temps))(*temps) if temps is not None else None
        self.n_temps = len(temps) if temps is not None else 1
        self.ids = (C.c_int32 * 4)(*ids) if ids is not None else None
        self.smp, self.con, self.hist, self.grp, self.req, self.keep = smp, con, hist, grp, req, keep

    def but(self, **kw):
        """a copy with some parts replaced"""
        p = Parts.__new__(Parts)
        p.__dict__.update(self.__dict__)
        for k, v in kw.items():
            if k == "temps":
                p.temps, p.n_temps = ((C.c_float * len(v))(*v), len(v)) if v is not None else (None, 1)
            else:
                setattr(p, k, v)
        return p


def _ref(x):
    return C.byref(x) if x is not None else None


def _ptr(x):
    return C.pointer(x) if x is not None else None


def old_call(lib, entry, p, outs, req_met, ws, ws_bytes, stream):
    """the status of the entry point ``sat_beam_search_<entry>`` (``sat_beam_search_batched`` ... ``_ensemble``); ``outs``: the eight
    output pointers in OUTPUTS' order.  An entry takes the parts it has arguments for."""
    tail = tuple(outs) + (ws, ws_bytes, stream)
    if entry == "ensemble":
        return lib.sat_beam_search_ensemble(_ref(p.ens), p.beamk, p.S, p.temps, p.n_temps, p.ids, _ref(p.con), _ref(p.hist), *tail)
    head = (_ref(p.dims), _ref(p.w), p.ann, p.beamk, p.S, p.temps, p.n_temps, p.ids)
    if entry == "batched":
        return lib.sat_beam_search_batched(*head, *tail)
    if entry == "sampled":
        return lib.sat_beam_search_sampled(*head, _ref(p.smp), *tail)
    if entry == "constrained":
        return lib.sat_beam_search_constrained(*head, _ref(p.smp), _ref(p.con), *tail)
    if entry == "history":
        return lib.sat_beam_search_history(*head, _ref(p.smp), _ref(p.con), _ref(p.hist), *tail)
    if entry == "groups":
        return lib.sat_beam_search_groups(*head, _ref(p.smp), _ref(p.con), _ref(p.hist), _ref(p.grp), *tail)
    assert entry == "required", entry
    return lib.sat_beam_search_required(*head, _ref(p.smp), _ref(p.con), _ref(p.hist), _ref(p.req), *(tuple(outs) + (req_met, ws, ws_bytes, stream)))


def descriptor(L, p):
    """the sat_beam_search_desc of the parts (it points into them: keep ``p`` alive)"""
    d = L.BeamSearchDesc(ann=p.ann, beamk=p.beamk, max_gen_length=p.S, n_temperatures=p.n_temps)
    for field, part in (("d", p.dims), ("w", p.w), ("ensemble", p.ens), ("sampling", p.smp), ("constraints", p.con), ("history", p.hist), ("groups", p.grp),
                        ("required", p.req)):
        if part is not None:
            setattr(d, field, _ptr(part))
    if p.temps is not None:
        d.temperatures_host = p.temps
    if p.ids is not None:
        d.special_ids_host = p.ids
    return d


def new_call(L, p, outs, req_met, ws, ws_bytes, stream):
    """the status of sat_beam_search on the same parts"""
    out = L.BeamSearchOut(*(tuple(outs) + (req_met,)))
    return L.lib().sat_beam_search(C.byref(descriptor(L, p)), C.byref(out), ws, ws_bytes, stream)
