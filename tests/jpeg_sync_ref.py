"""Numpy / Python restatement of the many-lane entropy decoding of sat_jpeg_decode_batch_ex (csrc/jpeg_decode.hip, "1b"),
independent of the kernels: the entropy-coded bytes of a restart-free picture are cut into subsequences of ``subseq_bytes`` raw
bytes (stuffed bytes count; the grid starts at the first data byte), and

1. speculative pass: lane i decodes from (first bit of subsequence i, slot 0, k 0) until a symbol would start at or past the
   subsequence's end; lane 0's state is the true one;
2. synchronisation: lane i + 1 decodes again from lane i's exit state until no exit state changes (a lane behind an error exit
   keeps its result; a lane handed a position at or past its end passes the state on);
3. an exclusive prefix sum of the completed blocks gives every lane its first block;
4. write pass: every lane decodes once more from its entry state and stores the non-zero AC coefficients and the DC differences;
5. a prefix sum of the DC differences per component in decode order, accumulated in int, stored as int16.

A decoder state is (raw bit position, slot within the MCU, zigzag index k; k == 0: a DC symbol comes next).  A raw bit position
never points into a stuffed 0x00: a lane that starts on one steps over it.  The result must equal jpeg_ref.decode_coefficients."""
import numpy as np

import jpeg_ref as R


class ParallelShort(ValueError):
    """the many-lane path came up short; the kernels then hand the picture to the serial lane"""


class Stream:
    """the raw bytes of a scan: the unstuffed 16-bit windows of jpeg_ref and the raw <-> unstuffed byte positions"""

    def __init__(self, scan):
        b = np.frombuffer(scan, np.uint8)
        self.n = b.size
        ff = np.flatnonzero(b[:-1] == 0xFF)
        if ff.size and np.any(b[ff + 1] != 0):
            raise ParallelShort("marker in the data")
        self.stuffed = np.zeros(b.size + 1, bool)
        self.stuffed[ff + 1] = True
        self.win, self.nbits = R.windows(scan)
        keep = np.flatnonzero(~self.stuffed[:-1])
        tail = b.size + np.arange(16)                                # positions past the end go on counting
        self.raw_of_u = np.concatenate([keep, tail]).tolist()
        u_of_raw = np.cumsum(~self.stuffed[:-1]) - 1                 # a stuffed byte: the 0xFF in front of it ...
        u_of_raw[self.stuffed[:-1]] += 1                             # ... so the byte behind it
        self.u_of_raw = u_of_raw.tolist() + [keep.size]

    def to_u(self, rawbit):
        byte, bit = rawbit >> 3, rawbit & 7
        assert not (bit and self.stuffed[byte])
        return 8 * self.u_of_raw[byte] + bit

    def to_raw(self, ubit):
        return 8 * self.raw_of_u[ubit >> 3] + (ubit & 7)


def lane(st, tabs, slots, ny, entry, end_byte, emit=None, first_block=0, total_blocks=None):
    """decode from ``entry`` = (raw bit, slot, k) until a symbol would start at or past raw byte ``end_byte``.
    -> (exit state, blocks completed, error or None); ``emit(block, k, value)`` gets the non-zero values (k == 0: a DC difference)"""
    rawbit, slot, k = entry
    if rawbit >> 3 >= end_byte:
        return entry, 0, None
    if rawbit & 7 == 0 and st.stuffed[rawbit >> 3]:
        rawbit += 8
    pos = st.to_u(rawbit)
    win, nblk, blk = st.win, 0, first_block
    dct, act = tabs
    while st.raw_of_u[pos >> 3] < end_byte and (total_blocks is None or blk < total_blocks):
        c = 0 if slot < ny else slot - ny + 1
        e = (act if k else dct)[c][win[pos]]
        if e == 0:
            return (st.to_raw(pos), slot, k), nblk, "bad Huffman code"
        pos += e >> 8
        sym = e & 255
        s = sym & 15
        if k == 0:
            if sym > 15:
                return (st.to_raw(pos), slot, k), nblk, "bad DC symbol"
        else:
            r = sym >> 4
            if s:
                k += r
                if k > 63:
                    return (st.to_raw(pos), slot, k), nblk, "coefficient index past 63"
            else:
                k = k + 15 if r == 15 and k + 15 < 63 else 63
        if s:
            x = win[pos] >> (16 - s)
            pos += s
            if emit is not None:
                emit(blk, k, x if x >= 1 << (s - 1) else x - (1 << s) + 1)
        k += 1
        if k > 63:
            if pos > st.nbits:
                return (st.to_raw(pos), slot, 63), nblk, "ran out of data"
            nblk, blk, k = nblk + 1, blk + 1, 0
            slot = slot + 1 if slot + 1 < slots else 0
    return (st.to_raw(pos), slot, k), nblk, None


def decode_coefficients(data, hd, subseq_bytes):
    """-> ((blocks, 64) int16 coefficients as jpeg_ref.decode_coefficients returns them, stats); raises ParallelShort where the
    kernels would fall back to the serial lane.  stats: subsequences, iterations (rounds run, the last one without a change),
    lane_decodes (speculative + synchronisation), max_lane_rounds (the most rounds in which one lane decoded again)."""
    assert len(hd.segments) == 1 and subseq_bytes >= 16 and subseq_bytes % 4 == 0
    scan = bytes(data[hd.data_start:hd.data_end])
    st = Stream(scan)
    geo = R.comp_geometry(hd)
    ny = geo[0]["hs"] * geo[0]["vs"]
    slots = ny + (2 if hd.components == 3 else 0)
    tabs = ([R.lut16(*t) for t in hd.dc], [R.lut16(*t) for t in hd.ac])
    nsub = -(-len(scan) // subseq_bytes)
    ends = [min(len(scan), (i + 1) * subseq_bytes) for i in range(nsub)]
    # 1. speculative pass
    entry = [(8 * i * subseq_bytes, 0, 0) for i in range(nsub)]
    res = [lane(st, tabs, slots, ny, entry[i], ends[i]) for i in range(nsub)]
    decodes, rounds = nsub, [0] * nsub
    # 2. synchronisation: every round reads the exit states of the round before
    iters, converged = 0, False
    while iters < nsub:
        iters += 1
        prev, changed = list(res), False
        for i in range(1, nsub):
            ex, _, err = prev[i - 1]
            if err is not None or ex == entry[i]:
                continue
            entry[i] = ex
            res[i] = lane(st, tabs, slots, ny, ex, ends[i])
            decodes += 1
            rounds[i] += 1
            changed = True
        if not changed:
            converged = True
            break
    if not converged:
        raise ParallelShort("iteration bound reached")
    # 3. block positions
    first = np.concatenate([[0], np.cumsum([r[1] for r in res])])
    nblk = [g["bw"] * g["bh"] for g in geo]
    base = np.concatenate([[0], np.cumsum(nblk)])
    total = int(base[-1])
    if int(first[-1]) != total:
        raise ParallelShort("%d blocks, the picture has %d" % (first[-1], total))
    # 4. write pass, jpeg_entropy_kernel's block addressing
    mx = geo[0]["bw"] // geo[0]["hs"]
    nat = R.J.NATURAL_ORDER.tolist()
    coef = np.zeros((total, 64), np.int64)

    def address(blk):
        m, slot = divmod(blk, slots)
        my_, mx_ = divmod(m, mx)
        if slot < ny:
            g = geo[0]
            return base[0] + (my_ * g["vs"] + slot // g["hs"]) * g["bw"] + mx_ * g["hs"] + slot % g["hs"]
        return base[slot - ny + 1] + my_ * mx + mx_

    def emit(blk, k, v):
        coef[address(blk), nat[k]] = v
    for i in range(nsub):
        if i and res[i - 1][0] != entry[i]:
            raise ParallelShort("lane %d: the chain is not verified" % i)
        if first[i] < total and first[i] % slots != entry[i][1]:
            raise ParallelShort("lane %d: slot" % i)
        _, _, err = lane(st, tabs, slots, ny, entry[i], ends[i], emit, int(first[i]), total)
        if err is not None:
            raise ParallelShort("lane %d: %s" % (i, err))
    # 5. DC prediction per component, in decode order
    order = [[], [], []]
    for blk in range(total):
        slot = blk % slots
        order[0 if slot < ny else slot - ny + 1].append(address(blk))
    for idx in order[:hd.components]:
        idx = np.array(idx, np.int64)
        coef[idx, 0] = np.cumsum(coef[idx, 0].astype(np.int32), dtype=np.int32).astype(np.int16)
    stats = dict(subsequences=nsub, iterations=iters, lane_decodes=decodes, max_lane_rounds=max(rounds))
    return coef.astype(np.int16), stats


def stuffed_boundaries(data, hd, subseq_bytes):
    """how many subsequence boundaries fall between a 0xFF and its stuffed 0x00"""
    scan = np.frombuffer(bytes(data[hd.data_start:hd.data_end]), np.uint8)
    b = np.arange(subseq_bytes, scan.size, subseq_bytes)
    return int(np.sum((scan[b - 1] == 0xFF) & (scan[b] == 0)))
