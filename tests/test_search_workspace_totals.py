"""CPU: the workspace totals of the caption decoders are pinned.  The per-image entry points and the batched searches lay their
workspaces out from one shared list of step buffers (csrc/decoder_search.hip, StepWs); the totals below were recorded from the library
as it was when each path still listed those buffers itself, so a buffer dropped, doubled or resized in either layout shows here.  The
queries are host arithmetic: nothing is launched and no pointer is followed."""
import ctypes as C

import pytest

B, D, A, M, N, V, S = 3, 24, 20, 12, 10, 37, 7          # sizes that are no multiple of the 256-byte rounding of a buffer

# (layers, L, K) -> totals in the order of _queries()
PINNED = {
    (1, 4, 1): (7936, 15104, 15616, 15616, 16128, 15616, 37888),
    (1, 4, 3): (9216, 25088, 25600, 26112, 26624, 26112, 62720),
    (1, 4, 6): (11776, 38912, 39936, 40448, 40960, 40448, 99328, 41728, 41728),
    (1, 49, 1): (11520, 26368, 26880, 26880, 27392, 26880, 49152),
    (1, 49, 3): (13312, 37376, 37888, 38400, 38912, 38400, 75008),
    (1, 49, 6): (16384, 52736, 53760, 54272, 54784, 54272, 113152, 55552, 55552),
    (2, 4, 1): (8192, 15616, 16128, 16128, 16640, 16128, 36608),
    (2, 4, 3): (9472, 26880, 27392, 27904, 28416, 27904, 61440),
    (2, 4, 6): (12032, 43264, 44288, 44800, 45312, 44800, 98048, 46080, 46080),
    (2, 49, 1): (11776, 26880, 27392, 27392, 27904, 27392, 47872),
    (2, 49, 3): (13568, 39168, 39680, 40192, 40704, 40192, 73728),
    (2, 49, 6): (16640, 57088, 58112, 58624, 59136, 58624, 111872, 59904, 59904),
}


def _dims(layers, Lc, K, **over):
    from sat_amd import decoder as Dk
    a = dict(dict(D=D, A=A, m=M, n=N), **over)
    return Dk.decoder_dims(B, K, 2, Lc, a["D"], a["A"], a["m"], a["n"], V, 0, True, 0, 0, layers=layers)


def _queries(layers, Lc, K):
    """the totals of one shape: per-image, plain, top-g, history, top-g with history, required words, a two-member ensemble with
    history; at K = 6 also two and three groups"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    d = _dims(layers, Lc, K)
    got = [lib.sat_decoder_infer_workspace_bytes(C.byref(d), K), lib.sat_beam_search_workspace_bytes(C.byref(d), K),
           lib.sat_beam_search_constrained_workspace_bytes(C.byref(d), K, 5), lib.sat_beam_search_history_workspace_bytes(C.byref(d), K, 0, S),
           lib.sat_beam_search_history_workspace_bytes(C.byref(d), K, 3, S), lib.sat_beam_search_required_workspace_bytes(C.byref(d), K, S, 2)]
    # the second member differs in L, D, n and layer count; one batch, one vocabulary
    other = _dims(3 - layers, 6, K, D=40, n=14)
    params, spot = L.DecoderParams(), C.c_float()
    ens = L.BeamEnsemble(members=2, combine=0)
    for i, dm in enumerate((d, other)):
        ens.dims[i], ens.params[i], ens.ann[i], ens.weight[i] = C.pointer(dm), C.pointer(params), C.addressof(spot), 0.5
    got.append(lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), K, S))
    if K == 6:
        got += [lib.sat_beam_search_groups_workspace_bytes(C.byref(d), K, 2, S), lib.sat_beam_search_groups_workspace_bytes(C.byref(d), K, 3, S)]
    return tuple(int(x) for x in got)


@pytest.mark.parametrize("shape", sorted(PINNED))
def test_workspace_totals_are_the_recorded_ones(shape):
    got = _queries(*shape)
    assert all(x > 0 for x in got), got
    assert got == PINNED[shape]
