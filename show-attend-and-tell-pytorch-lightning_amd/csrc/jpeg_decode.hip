// Baseline JPEG decoding on device: util.py:136-137's Image.open(f).convert("RGB") for the files sat_amd/jpeg.py classifies
// as GPU-decodable, bit exact with Pillow's libjpeg-turbo at its defaults (JDCT_ISLOW, fancy upsampling, no block smoothing).
//   1. entropy decoding: one thread (lane 0 of a wave) per picture and restart segment.  Huffman codes through a 9-bit lookup
//      table plus libjpeg's maxcode / valoffset search for longer codes; the picture's tables sit in LDS.  The coefficient
//      blocks were cleared first, so only the non-zero coefficients are stored (int16, natural order).
//      A restart-free picture above a size threshold is instead cut into subsequences with a lane each that synchronise on the
//      device (section 1b below); what comes out is the same.
//   2. dequantisation + jidctint.c's jpeg_idct_islow, one thread per 8x8 block, operation for operation, output through
//      libjpeg's range_limit table (a wrap, not a clamp, for overshooting coefficients).
//   3. jdsample.c's fancy upsampling (h2v1, h2v2; plain replication when the chroma is at most 2 samples wide) and jdcolor.c's
//      fixed-point YCbCr->RGB, one thread per output pixel.
// Integer arithmetic only.  Every read is bounded by the segment and the table arrays, every write by the picture's blocks
// and its (height, width, 3) output; a bad stream sets the picture's status word and leaves the other pictures alone.
#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {
namespace {

constexpr int JPEG_LOOKAHEAD = 9;
constexpr int JPEG_BAD_CODE = 1, JPEG_OUT_OF_DATA = 2, JPEG_BAD_INDEX = 4, JPEG_BAD_SEGMENT = 8, JPEG_MARKER = 16;

__constant__ uint8_t k_natural_order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// geometry of component c of a picture: its blocks per row / column in the coefficient array and the samples that are real
struct CompGeom {
    int bw, bh;          // blocks (every block of every MCU: the array libjpeg's coefficient controller holds)
    int dw, dh;          // downsampled_width / downsampled_height
    int hs, vs;          // this component's sampling factors
};

__host__ __device__ inline CompGeom comp_geom(const sat_jpeg_desc& d, int c) {
    CompGeom g;
    if (d.components == 1) {
        g.bw = (d.width + 7) / 8; g.bh = (d.height + 7) / 8;
        g.dw = d.width; g.dh = d.height; g.hs = g.vs = 1;
        return g;
    }
    const int mx = (d.width + 8 * d.h_samp - 1) / (8 * d.h_samp), my = (d.height + 8 * d.v_samp - 1) / (8 * d.v_samp);
    g.hs = c == 0 ? d.h_samp : 1;
    g.vs = c == 0 ? d.v_samp : 1;
    g.bw = mx * g.hs; g.bh = my * g.vs;
    g.dw = (d.width * g.hs + d.h_samp - 1) / d.h_samp;          // jdinput.c: ceil(image_width * h / max_h)
    g.dh = (d.height * g.vs + d.v_samp - 1) / d.v_samp;
    return g;
}

__host__ __device__ inline long picture_blocks(const sat_jpeg_desc& d) {
    long total = 0;
    for (int c = 0; c < d.components; ++c) { CompGeom g = comp_geom(d, c); total += (long)g.bw * g.bh; }
    return total;
}

__host__ __device__ inline long picture_mcus(const sat_jpeg_desc& d) {
    if (d.components == 1) return (long)((d.width + 7) / 8) * ((d.height + 7) / 8);
    return (long)((d.width + 8 * d.h_samp - 1) / (8 * d.h_samp)) * ((d.height + 8 * d.v_samp - 1) / (8 * d.v_samp));
}

// ---------------------------------------------------------------------------------------------------------------- 1. entropy
// Bit reader over one restart segment: bytes [pos, end) of the picture's data, 0xFF00 -> 0xFF.  Past the end (or at a
// marker) it shifts in zero bytes, as libjpeg does, and counts them: consuming any of those bits is "ran out of data".
struct BitReader {
    const uint8_t* base;     // the compressed buffer
    long abs0;               // absolute offset of the picture's data
    long pos, end;           // relative to abs0
    long limit;              // compressed_bytes: bound for the aligned word loads
    uint64_t buf;            // bits, left-aligned
    int cnt;                 // valid bits in buf
    int fill;                // zero bytes shifted in past the end
    int flags;
    long word_idx;
    uint32_t word;

    __device__ inline int byte_at(long rel) {
        const long a = abs0 + rel;
        const long w = a >> 2;
        if (w != word_idx) {
            if ((w << 2) + 4 <= limit) word = *reinterpret_cast<const uint32_t*>(base + (w << 2));
            else {
                word = 0;
                for (int k = 0; k < 4 && (w << 2) + k < limit; ++k) word |= (uint32_t)base[(w << 2) + k] << (8 * k);
            }
            word_idx = w;
        }
        return (word >> (8 * (a & 3))) & 0xFF;
    }

    __device__ inline void refill() {
        while (cnt <= 56) {
            int v = 0;
            if (pos < end) {
                v = byte_at(pos++);
                if (v == 0xFF) {
                    const int nx = pos < end ? byte_at(pos) : 0;
                    if (nx == 0) ++pos;
                    else { flags |= JPEG_MARKER; pos = end; v = 0; ++fill; }
                }
            } else {
                ++fill;
            }
            buf |= (uint64_t)v << (56 - cnt);
            cnt += 8;
            if (fill > 64) fill = 64;       // enough to flag it; keeps the counter bounded
        }
    }

    __device__ inline uint32_t peek(int n) { return (uint32_t)(buf >> (64 - n)); }
    __device__ inline void skip(int n) { buf <<= n; cnt -= n; }
    __device__ inline bool overrun() const { return fill * 8 > cnt; }
};

__device__ inline int huff_decode(BitReader& br, const sat_jpeg_htable& t) {
    br.refill();
    const int e = t.lookup[br.peek(JPEG_LOOKAHEAD)];
    if (e) { br.skip(e >> 8); return e & 0xFF; }
    const uint32_t w = br.peek(16);
    for (int l = JPEG_LOOKAHEAD + 1; l <= 16; ++l) {
        const int code = (int)(w >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int idx = code + t.valoffset[l];
            if (idx < 0 || idx > 255) break;
            br.skip(l);
            return t.huffval[idx];
        }
    }
    br.flags |= JPEG_BAD_CODE;
    return -1;
}

__device__ inline int receive_extend(BitReader& br, int s) {
    if (s == 0) return 0;
    br.refill();
    const int r = (int)br.peek(s);
    br.skip(s);
    return r < (1 << (s - 1)) ? r + (int)((~0u << s) + 1u) : r;       // HUFF_EXTEND
}

// the picture's DC / AC tables (component c: tabs[2 c], tabs[2 c + 1]) into LDS, by every thread of the block
__device__ __forceinline__ void load_tables(sat_jpeg_htable* tabs, const sat_jpeg_desc& d, const sat_jpeg_htable* __restrict__ huff) {
    const int nt = 2 * d.components;
    for (int t = 0; t < nt; ++t) {
        const int idx = (t & 1) ? d.ac_table[t >> 1] : d.dc_table[t >> 1];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + idx);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tabs[t]);
        for (int k = threadIdx.x; k < (int)(sizeof(sat_jpeg_htable) / 4); k += blockDim.x) dst[k] = src[k];
    }
    __syncthreads();
}

// the serial lane: restart segment `seg` of picture p, one thread (inlined into its kernels, so that `tabs` stays an LDS address)
__device__ __forceinline__ void entropy_serial_lane(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc& d, int p, int seg,
                                           const sat_jpeg_htable* tabs, int16_t* __restrict__ coefs, int* __restrict__ status) {
    const uint32_t* segtab = reinterpret_cast<const uint32_t*>(comp + d.segments_offset);
    const long s0 = segtab[2 * seg], s1 = segtab[2 * seg + 1];
    if (s0 > s1 || s1 > d.data_bytes) { atomicOr(status + p, JPEG_BAD_SEGMENT); return; }
    BitReader br;
    br.base = comp; br.abs0 = d.data_offset; br.pos = s0; br.end = s1; br.limit = comp_bytes;
    br.buf = 0; br.cnt = 0; br.fill = 0; br.flags = 0; br.word_idx = -1; br.word = 0;

    const long total = picture_mcus(d);
    const long m0 = d.restart_interval ? (long)seg * d.restart_interval : 0;
    const long m1 = d.restart_interval ? min(total, m0 + d.restart_interval) : total;
    // per-component values as scalars (a run-time index into small arrays would put them in scratch memory)
    const CompGeom g0 = comp_geom(d, 0);
    const int hs = g0.hs, vs = g0.vs, bw0 = g0.bw;
    const int mx = d.components == 1 ? bw0 : bw0 / hs;
    const int bwc = mx;                                        // chroma: one block per MCU
    const long base0 = d.block_offset, base1 = base0 + (long)g0.bw * g0.bh, base2 = base1 + (d.components == 3 ? (long)mx * (g0.bh / vs) : 0);
    const int ny = hs * vs, slots = ny + (d.components == 3 ? 2 : 0);
    int dc0 = 0, dc1 = 0, dc2 = 0;
    for (long m = m0; m < m1 && !(br.flags & ~JPEG_MARKER); ++m) {
        const int mcu_x = (int)(m % mx), mcu_y = (int)(m / mx);
        for (int slot = 0; slot < slots && !(br.flags & ~JPEG_MARKER); ++slot) {
            const int c = slot < ny ? 0 : slot - ny + 1;
            long bi;
            if (c == 0) bi = base0 + (long)(mcu_y * vs + slot / hs) * bw0 + mcu_x * hs + slot % hs;
            else bi = (c == 1 ? base1 : base2) + (long)mcu_y * bwc + mcu_x;
            int16_t* blk = coefs + bi * 64;
            const sat_jpeg_htable& dct = tabs[2 * c];
            const sat_jpeg_htable& act = tabs[2 * c + 1];
            int s = huff_decode(br, dct);
            if (s > 15) br.flags |= JPEG_BAD_CODE;
            if (s >= 0 && s <= 15) {
                const int diff = receive_extend(br, s);
                const int dcv = (c == 0 ? dc0 : (c == 1 ? dc1 : dc2)) + diff;
                if (c == 0) dc0 = dcv; else if (c == 1) dc1 = dcv; else dc2 = dcv;
                if (dcv) blk[0] = (int16_t)dcv;
                for (int k = 1; k < 64; ++k) {
                    const int rs = huff_decode(br, act);
                    if (rs < 0) break;
                    const int r = rs >> 4;
                    s = rs & 15;
                    if (s) {
                        k += r;
                        if (k > 63) { br.flags |= JPEG_BAD_INDEX; break; }
                        blk[k_natural_order[k]] = (int16_t)receive_extend(br, s);
                    } else {
                        if (r != 15) break;
                        k += 15;
                    }
                }
            }
            if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
        }
    }
    if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
    if (br.flags) atomicOr(status + p, br.flags);
}

// Per-picture control words of the parallel path (PAR_CTRL int32 each, in the workspace; written by jpeg_par_setup_kernel)
constexpr int PAR_CTRL = 8;
constexpr int PC_PATH = 0, PC_BASE = 1, PC_NSUB = 2, PC_ITERS = 3, PC_FAIL = 4, PC_WFAIL = 5;      // FAIL: before the write pass; WFAIL: in it

// One lane per picture and restart segment.  `ctrl` (may be null): the pictures the parallel path below has taken are skipped.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                          int n, const sat_jpeg_htable* __restrict__ huff, int16_t* __restrict__ coefs,
                                                          int* __restrict__ status, const int* __restrict__ ctrl) {
    __shared__ sat_jpeg_htable tabs[6];
    const int seg_global = blockIdx.x;
    int lo = 0, hi = n - 1;                                   // picture: last one whose segment_base <= seg_global
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].segment_base <= seg_global) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    const sat_jpeg_desc& d = desc[p];                        // a reference: a local copy's arrays would live in scratch memory
    const int seg = seg_global - d.segment_base;
    if (seg < 0 || seg >= d.n_segments) return;
    if (ctrl && ctrl[p * PAR_CTRL + PC_PATH]) return;
    load_tables(tabs, d, huff);
    if (threadIdx.x != 0) return;
    entropy_serial_lane(comp, comp_bytes, d, p, seg, tabs, coefs, status);
}

// -------------------------------------------------------------------------------------------------- 1b. entropy, many lanes
// A restart-free picture (one segment) of at least parallel_min_bytes is cut into subsequences of subseq_bytes raw bytes,
// measured from data_offset, stuffed bytes counted.  A decoder state is (bit position in the raw bytes, slot within the MCU,
// zigzag index k; k == 0: a DC symbol comes next).  jpeg_par_spec_kernel: lane i decodes subsequence i from (its first bit,
// slot 0, k 0) until a symbol would start at or past the subsequence's end; lane 0's state is the true one.
// jpeg_par_sync_kernel (one workgroup per picture): lane i + 1 decodes again from lane i's exit state until no exit state
// changes, then the exclusive prefix sum of the completed blocks gives every lane its first block.  jpeg_par_write_kernel:
// every lane decodes once more from its verified entry state and stores the non-zero AC coefficients and the DC differences
// with jpeg_entropy_kernel's block addressing.  jpeg_par_dc_kernel: the prefix sum of the DC differences per component in
// decode order.  A picture on which any of this comes up short (a marker in the data, an unverified chain, a block count that
// is not the picture's, a flag in the write pass) is cleared and decoded by the serial lane in jpeg_par_finish_kernel, so its
// status word and pixels are the serial path's.
// A bit position is canonical: the byte after a 0xFF is never pointed at (the reader skips it when it loads the 0xFF, and a
// lane that starts on it steps over it), so equal decoder states compare equal.
constexpr int PAR_THREADS = 256;            // spec / write / dc kernels
constexpr int PAR_SYNC_THREADS = 1024;      // one workgroup per picture
constexpr long PAR_MAX_BYTES = 1L << 27;    // bit positions stay below 2^30
constexpr uint64_t ST_ERR = 1ull << 63;

__host__ __device__ inline uint64_t st_pack(uint32_t bitpos, int slot, int k) { return (uint64_t)bitpos | ((uint64_t)slot << 32) | ((uint64_t)k << 40); }
__host__ __device__ inline uint32_t st_pos(uint64_t s) { return (uint32_t)s; }
__host__ __device__ inline int st_slot(uint64_t s) { return (int)((s >> 32) & 0xFF); }
__host__ __device__ inline int st_k(uint64_t s) { return (int)((s >> 40) & 0xFF); }

__host__ __device__ inline bool par_takes(const sat_jpeg_desc& d, long min_bytes) {
    return d.n_segments == 1 && d.data_bytes > 0 && d.data_bytes >= min_bytes && d.data_bytes <= PAR_MAX_BYTES;
}

// Bit reader of a lane over the whole data [0, end) of the picture.  `pos` is the next raw byte; past the end it goes on counting
// while zero bytes are shifted in.  `stuff` remembers, for the last bytes loaded (bit 0: the latest), whether a stuffed byte
// followed, so that the raw position of the next unread bit can be told from pos and cnt.
struct LaneReader {
    const uint8_t* base;
    long abs0, limit;
    int pos, end;
    uint64_t buf;
    int cnt;
    uint32_t stuff;
    int flags;
    long word_idx;
    uint32_t word;

    __device__ inline int byte_at(int rel) {
        const long a = abs0 + rel;
        const long w = a >> 2;
        if (w != word_idx) {
            if ((w << 2) + 4 <= limit) word = *reinterpret_cast<const uint32_t*>(base + (w << 2));
            else {
                word = 0;
                for (int k = 0; k < 4 && (w << 2) + k < limit; ++k) word |= (uint32_t)base[(w << 2) + k] << (8 * k);
            }
            word_idx = w;
        }
        return (word >> (8 * (a & 3))) & 0xFF;
    }

    __device__ inline void refill() {
        while (cnt <= 56) {
            int v = 0, st = 0;
            if (pos < end) {
                v = byte_at(pos);
                if (v == 0xFF) {
                    const int nx = pos + 1 < end ? byte_at(pos + 1) : 0;
                    if (nx == 0) { ++pos; st = 1; }
                    else { flags |= JPEG_MARKER; end = pos; v = 0; }        // the data ends here; the picture goes to the serial lane
                }
            }
            ++pos;
            buf |= (uint64_t)v << (56 - cnt);
            cnt += 8;
            stuff = (stuff << 1) | st;
        }
    }

    __device__ inline void start(uint32_t bitpos) {
        pos = (int)(bitpos >> 3);
        const int bit = (int)(bitpos & 7);
        buf = 0; cnt = 0; stuff = 0; flags = 0; word_idx = -1; word = 0;
        if (bit == 0 && pos > 0 && pos < end && byte_at(pos) == 0 && byte_at(pos - 1) == 0xFF) ++pos;      // on a stuffed byte
        refill();
        skip(bit);
    }

    // raw bit position of the next unread bit
    __device__ inline uint32_t bitpos() const {
        const int nb = (cnt + 7) >> 3;
        const int first = pos - nb - __popc(stuff & ((1u << nb) - 1u));
        return ((uint32_t)first << 3) + (uint32_t)((8 - (cnt & 7)) & 7);
    }
    __device__ inline uint32_t peek(int n) { return (uint32_t)(buf >> (64 - n)); }
    __device__ inline void skip(int n) { buf <<= n; cnt -= n; }
};

// block addressing of jpeg_entropy_kernel, for the write and DC passes
struct BlockMap {
    int hs, vs, bw0, mx, ny, slots;
    long base0, base1, base2, total;

    __device__ inline void init(const sat_jpeg_desc& d) {
        const CompGeom g0 = comp_geom(d, 0);
        hs = g0.hs; vs = g0.vs; bw0 = g0.bw;
        mx = d.components == 1 ? bw0 : bw0 / hs;
        base0 = d.block_offset; base1 = base0 + (long)g0.bw * g0.bh; base2 = base1 + (d.components == 3 ? (long)mx * (g0.bh / vs) : 0);
        ny = hs * vs; slots = ny + (d.components == 3 ? 2 : 0);
        total = picture_mcus(d) * slots;
    }
    __device__ inline long block(long m, int slot) const {
        const int mcu_x = (int)(m % mx), mcu_y = (int)(m / mx);
        if (slot < ny) return base0 + (long)(mcu_y * vs + slot / hs) * bw0 + mcu_x * hs + slot % hs;
        return (slot == ny ? base1 : base2) + (long)mcu_y * mx + mcu_x;
    }
};

// One lane: decode from `entry` until a symbol would start at or past byte `end_byte` (or, when writing, until the picture's
// blocks are done).  One symbol per iteration, DC or AC by k, so the lanes of a wave reconverge every symbol; a symbol takes at
// least one bit, so the loop makes at most 8 * (end_byte - first byte) iterations whatever the bytes are.
// Returns the exit state (ST_ERR set on a bad code, an index past 63 or a block that ran out of data) and the blocks completed.
template <bool WRITE>
__device__ __forceinline__ uint64_t lane_decode(LaneReader& br, const sat_jpeg_htable* tabs, int ny, int slots, uint64_t entry, int end_byte, int* nblk_out,
                                       const BlockMap* bm, long blk_abs, int16_t* __restrict__ coefs) {
    *nblk_out = 0;
    if ((int)(st_pos(entry) >> 3) >= end_byte) return entry;            // handed a position past this subsequence: pass it on
    int slot = st_slot(entry), k = st_k(entry), nblk = 0;
    br.start(st_pos(entry));
    const uint32_t data_bits = (uint32_t)br.end << 3;
    int16_t* blk = nullptr;
    if (WRITE && blk_abs < bm->total) blk = coefs + bm->block(blk_abs / slots, (int)(blk_abs % slots)) * 64;
    bool err = false;
    for (;;) {
        if ((int)(br.bitpos() >> 3) >= end_byte) break;
        if (WRITE && blk_abs >= bm->total) break;
        br.refill();                                                      // >= 57 bits: a code (16) and its value bits (15)
        const int c = slot < ny ? 0 : slot - ny + 1;
        const sat_jpeg_htable& t = tabs[2 * c + (k ? 1 : 0)];
        int sym = -1;
        const int e = t.lookup[br.peek(JPEG_LOOKAHEAD)];
        if (e >> 8) { br.skip(e >> 8); sym = e & 0xFF; }
        else if (!e) {
            const uint32_t w = br.peek(16);
            for (int l = JPEG_LOOKAHEAD + 1; l <= 16; ++l) {
                const int code = (int)(w >> (16 - l));
                if (code <= t.maxcode[l]) {
                    const int idx = code + t.valoffset[l];
                    if (idx >= 0 && idx <= 255) { br.skip(l); sym = t.huffval[idx]; }
                    break;
                }
            }
        }
        if (sym < 0) { br.flags |= JPEG_BAD_CODE; err = true; break; }
        int s = sym & 15, v = 0;
        if (k == 0) {
            if (sym > 15) { br.flags |= JPEG_BAD_CODE; err = true; break; }
        } else {
            const int r = sym >> 4;
            if (s) {
                k += r;
                if (k > 63) { br.flags |= JPEG_BAD_INDEX; err = true; break; }
            } else {
                k = (r == 15 && k + 15 < 63) ? k + 15 : 63;               // ZRL: 16 zeros; EOB (or a ZRL past the end): the block is done
            }
        }
        if (s) {
            const int r = (int)br.peek(s);
            br.skip(s);
            v = r < (1 << (s - 1)) ? r + (int)((~0u << s) + 1u) : r;      // HUFF_EXTEND
            if (WRITE) blk[k_natural_order[k]] = (int16_t)v;              // k == 0: the DC difference
        }
        if (++k > 63) {
            if (br.bitpos() > data_bits) { br.flags |= JPEG_OUT_OF_DATA; err = true; break; }
            ++nblk; k = 0;
            if (++slot == slots) slot = 0;
            if (WRITE) {
                ++blk_abs;
                if (blk_abs < bm->total) blk = coefs + bm->block(blk_abs / slots, (int)(blk_abs % slots)) * 64;
            }
        }
    }
    *nblk_out = nblk;
    return st_pack(br.bitpos(), slot, k) | (err ? ST_ERR : 0);
}

// ctrl[p]: does picture p take the parallel path, its first subsequence in the state arrays and its subsequences.  One block.
__global__ __launch_bounds__(PAR_THREADS) void jpeg_par_setup_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                                      int n, int subseq, long min_bytes, long cap, int* __restrict__ ctrl) {
    __shared__ long part[PAR_THREADS];
    const int per = (n + PAR_THREADS - 1) / PAR_THREADS;
    const int p0 = min(n, (int)threadIdx.x * per), p1 = min(n, p0 + per);
    auto subs = [&](int p) -> long {
        const sat_jpeg_desc& d = desc[p];
        if (!par_takes(d, min_bytes)) return 0;
        if (d.data_offset < 0 || d.data_offset + d.data_bytes > comp_bytes || d.segments_offset < 0 || d.segments_offset + 8 > comp_bytes) return 0;
        const uint32_t* segtab = reinterpret_cast<const uint32_t*>(comp + d.segments_offset);
        if (segtab[0] != 0 || (long)segtab[1] != d.data_bytes) return 0;          // the serial lane's segment is not the whole data
        return (d.data_bytes + subseq - 1) / subseq;
    };
    long sum = 0;
    for (int p = p0; p < p1; ++p) sum += subs(p);
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long run = 0;
        for (int t = 0; t < PAR_THREADS; ++t) { const long v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    long base = part[threadIdx.x];
    for (int p = p0; p < p1; ++p) {
        long ns = subs(p);
        if (base + ns > cap) ns = 0;                                             // never past the state arrays
        int* c = ctrl + (long)p * PAR_CTRL;
        c[PC_PATH] = ns > 0; c[PC_BASE] = (int)base; c[PC_NSUB] = (int)ns; c[PC_ITERS] = 0; c[PC_FAIL] = 0; c[5] = c[6] = c[7] = 0;
        base += ns;
    }
}

__device__ inline void lane_reader_init(LaneReader& br, const uint8_t* comp, long comp_bytes, const sat_jpeg_desc& d) {
    br.base = comp; br.abs0 = d.data_offset; br.limit = comp_bytes; br.end = (int)d.data_bytes;
}

// is there a marker (0xFF followed by anything but 0x00) that starts in bytes [b0, b1) of the data?
__device__ inline bool has_marker(LaneReader& br, int b0, int b1, int data_bytes) {
    br.word_idx = -1; br.word = 0;
    bool found = false;
    for (int b = b0; b < b1;) {
        const long a = br.abs0 + b;
        br.byte_at(b);                                                            // loads the word that holds byte b
        const uint32_t x = ~br.word;
        const int in_word = 4 - (int)(a & 3);
        if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) { b += in_word; continue; }       // no 0xFF in this word
        const int stop = min(b1, b + in_word);
        for (; b < stop; ++b)
            if (br.byte_at(b) == 0xFF && b + 1 < data_bytes && br.byte_at(b + 1) != 0) found = true;
    }
    return found;
}

__global__ __launch_bounds__(PAR_THREADS) void jpeg_par_spec_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                                     const sat_jpeg_htable* __restrict__ huff, int subseq, int* __restrict__ ctrl,
                                                                     uint64_t* __restrict__ st_exit, uint64_t* __restrict__ st_entry, int* __restrict__ nblk) {
    __shared__ sat_jpeg_htable tabs[6];
    const int p = blockIdx.y;
    int* c = ctrl + (long)p * PAR_CTRL;
    const int nsub = c[PC_NSUB], base = c[PC_BASE];
    if (!c[PC_PATH] || (long)blockIdx.x * PAR_THREADS >= nsub) return;
    const sat_jpeg_desc& d = desc[p];
    load_tables(tabs, d, huff);
    const int ny = d.components == 1 ? 1 : d.h_samp * d.v_samp, slots = ny + (d.components == 3 ? 2 : 0);
    LaneReader br;
    lane_reader_init(br, comp, comp_bytes, d);
    const int data_bytes = br.end;
    for (long i = (long)blockIdx.x * PAR_THREADS + threadIdx.x; i < nsub; i += (long)gridDim.x * PAR_THREADS) {
        const int b0 = (int)(i * subseq), b1 = min(data_bytes, b0 + subseq);
        if (has_marker(br, b0, b1, data_bytes)) atomicOr(c + PC_FAIL, 1);
        const uint64_t entry = st_pack((uint32_t)b0 << 3, 0, 0);
        int nb;
        br.end = data_bytes;
        const uint64_t ex = lane_decode<false>(br, tabs, ny, slots, entry, b1, &nb, nullptr, 0, nullptr);
        st_entry[base + i] = entry; st_exit[base + i] = ex; nblk[base + i] = nb;
    }
}

__global__ __launch_bounds__(PAR_SYNC_THREADS) void jpeg_par_sync_kernel(const uint8_t* __restrict__ comp, long comp_bytes,
                                                                          const sat_jpeg_desc* __restrict__ desc, const sat_jpeg_htable* __restrict__ huff,
                                                                          int subseq, int* __restrict__ ctrl, uint64_t* st_exit, uint64_t* st_entry, int* nblk,
                                                                          int* __restrict__ blk_base) {
    __shared__ sat_jpeg_htable tabs[6];
    __shared__ int part[PAR_SYNC_THREADS];
    const int p = blockIdx.x;
    int* c = ctrl + (long)p * PAR_CTRL;
    const int nsub = c[PC_NSUB], base = c[PC_BASE];
    if (!c[PC_PATH] || c[PC_FAIL]) return;                                      // the whole block: no barrier is left waiting
    const sat_jpeg_desc& d = desc[p];
    load_tables(tabs, d, huff);
    const int ny = d.components == 1 ? 1 : d.h_samp * d.v_samp, slots = ny + (d.components == 3 ? 2 : 0);
    LaneReader br;
    lane_reader_init(br, comp, comp_bytes, d);
    const int data_bytes = br.end;
    uint64_t* ex = st_exit + base;
    uint64_t* en = st_entry + base;
    // Every round, lane i decodes again if lane i - 1's exit state is not the entry state it last used.  The exit words are read
    // while other lanes of the round may store them (8-byte atomic accesses); a round in which no lane stored anything has read
    // stable words, so at its end ex[i - 1] == en[i] and ex[i] = decode(en[i]) for every lane behind a good predecessor.  After
    // round r lanes 0 ... r hold their true states, hence at most nsub rounds.
    int iters = 0;
    bool converged = false;
    while (iters < nsub) {
        ++iters;
        int changed = 0;
        for (int i = 1 + threadIdx.x; i < nsub; i += PAR_SYNC_THREADS) {
            const uint64_t e = __atomic_load_n(ex + i - 1, __ATOMIC_RELAXED);
            if ((e & ST_ERR) || e == en[i]) continue;
            int nb;
            br.end = data_bytes;
            const uint64_t out = lane_decode<false>(br, tabs, ny, slots, e, min(data_bytes, (i + 1) * subseq), &nb, nullptr, 0, nullptr);
            en[i] = e; nblk[base + i] = nb;
            __atomic_store_n(ex + i, out, __ATOMIC_RELAXED);
            changed = 1;
        }
        if (!__syncthreads_or(changed)) { converged = true; break; }
    }
    // exclusive prefix sum of the completed blocks: a contiguous run of subsequences per thread
    const int per = (nsub + PAR_SYNC_THREADS - 1) / PAR_SYNC_THREADS;
    const int i0 = min(nsub, (int)threadIdx.x * per), i1 = min(nsub, i0 + per);
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += nblk[base + i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < PAR_SYNC_THREADS; off <<= 1) {
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int i = i0; i < i1; ++i) { blk_base[base + i] = run; run += nblk[base + i]; }
    if (threadIdx.x == PAR_SYNC_THREADS - 1) {
        const long total = picture_mcus(d) * slots;
        c[PC_ITERS] = iters;
        if (!converged || (long)part[threadIdx.x] != total) atomicOr(c + PC_FAIL, 2);
    }
}

__global__ __launch_bounds__(PAR_THREADS) void jpeg_par_write_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                                      const sat_jpeg_htable* __restrict__ huff, int subseq, int* __restrict__ ctrl,
                                                                      const uint64_t* __restrict__ st_exit, const uint64_t* __restrict__ st_entry,
                                                                      const int* __restrict__ blk_base, int16_t* __restrict__ coefs) {
    __shared__ sat_jpeg_htable tabs[6];
    const int p = blockIdx.y;
    int* c = ctrl + (long)p * PAR_CTRL;
    const int nsub = c[PC_NSUB], base = c[PC_BASE];
    if (!c[PC_PATH] || c[PC_FAIL] || (long)blockIdx.x * PAR_THREADS >= nsub) return;
    const sat_jpeg_desc& d = desc[p];
    load_tables(tabs, d, huff);
    BlockMap bm;
    bm.init(d);
    LaneReader br;
    lane_reader_init(br, comp, comp_bytes, d);
    const int data_bytes = br.end;
    for (long i = (long)blockIdx.x * PAR_THREADS + threadIdx.x; i < nsub; i += (long)gridDim.x * PAR_THREADS) {
        const uint64_t entry = st_entry[base + i];
        const long first = blk_base[base + i];
        // the chain is verified only where a lane's entry is its predecessor's exit (an error exit never is) and the slot fits the block
        bool bad = (i > 0 && st_exit[base + i - 1] != entry) || (first < bm.total && (int)(first % bm.slots) != st_slot(entry));
        if (!bad) {
            int nb;
            br.end = data_bytes; br.flags = 0;
            lane_decode<true>(br, tabs, bm.ny, bm.slots, entry, (int)min((long)data_bytes, (i + 1) * subseq), &nb, &bm, first, coefs);
            bad = br.flags != 0;
        }
        if (bad) atomicOr(c + PC_WFAIL, 1);
    }
}

// blk[0] of every block holds its DC difference: replace it by the running sum per component, in decode order
__global__ __launch_bounds__(PAR_THREADS) void jpeg_par_dc_kernel(const sat_jpeg_desc* __restrict__ desc, const int* __restrict__ ctrl, int16_t* __restrict__ coefs) {
    __shared__ int part[PAR_THREADS];
    const int p = blockIdx.y, comp_i = blockIdx.x;
    const int* c = ctrl + (long)p * PAR_CTRL;
    const sat_jpeg_desc& d = desc[p];
    if (!c[PC_PATH] || c[PC_FAIL] || c[PC_WFAIL] || comp_i >= d.components) return;
    BlockMap bm;
    bm.init(d);
    const long mcus = bm.total / bm.slots;
    const int per_mcu = comp_i == 0 ? bm.ny : 1, slot0 = comp_i == 0 ? 0 : bm.ny + comp_i - 1;
    const long nb = mcus * per_mcu;
    const long per = (nb + PAR_THREADS - 1) / PAR_THREADS;
    const long j0 = min(nb, (long)threadIdx.x * per), j1 = min(nb, j0 + per);
    unsigned sum = 0;                                                             // int arithmetic modulo 2^32, as the serial lane's
    for (long j = j0; j < j1; ++j) sum += (unsigned)(int)coefs[bm.block(j / per_mcu, slot0 + (int)(j % per_mcu)) * 64];
    part[threadIdx.x] = (int)sum;
    __syncthreads();
    for (int off = 1; off < PAR_THREADS; off <<= 1) {
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] = (int)((unsigned)part[threadIdx.x] + (unsigned)v);
        __syncthreads();
    }
    unsigned run = (unsigned)part[threadIdx.x] - sum;
    for (long j = j0; j < j1; ++j) {
        int16_t* blk = coefs + bm.block(j / per_mcu, slot0 + (int)(j % per_mcu)) * 64;
        const int diff = blk[0];
        run += (unsigned)diff;
        if ((int)run != diff) blk[0] = (int16_t)(int)run;
    }
}

// One block per picture.  A picture the parallel path gave up on: clear its blocks and decode it on the serial lane.  Every
// picture: its info words (path 0 serial, 1 parallel, 2 parallel abandoned for the serial lane; subsequences; iterations; 0).
__global__ __launch_bounds__(64) void jpeg_par_finish_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                              const sat_jpeg_htable* __restrict__ huff, const int* __restrict__ ctrl,
                                                              int16_t* __restrict__ coefs, int* __restrict__ status, int* __restrict__ info) {
    __shared__ sat_jpeg_htable tabs[6];
    const int p = blockIdx.x;
    const int* c = ctrl + (long)p * PAR_CTRL;
    const bool redo = c[PC_PATH] && (c[PC_FAIL] || c[PC_WFAIL]);
    if (info && threadIdx.x == 0) {
        info[4 * p] = c[PC_PATH] ? (redo ? 2 : 1) : 0; info[4 * p + 1] = c[PC_NSUB]; info[4 * p + 2] = c[PC_ITERS]; info[4 * p + 3] = 0;
    }
    if (!redo) return;
    const sat_jpeg_desc& d = desc[p];
    uint4* blocks = reinterpret_cast<uint4*>(coefs + d.block_offset * 64);
    const long n16 = picture_blocks(d) * 8;
    for (long k = threadIdx.x; k < n16; k += 64) blocks[k] = make_uint4(0, 0, 0, 0);
    load_tables(tabs, d, huff);                                                   // ends in a barrier: the blocks are clear
    if (threadIdx.x != 0) return;
    entropy_serial_lane(comp, comp_bytes, d, p, 0, tabs, coefs, status);
}

// -------------------------------------------------------------------------------------------------- 1c. entropy, progressive
// sat_jpeg_decode_progressive_batch: the scans of a progressive picture fill the same coefficient array, a band and a bit position
// at a time.  One launch per dependency level, one workgroup (one wave) per scan and restart segment.  Lane 0 is the serial bit
// reader and runs jdphuff.c's arithmetic; the other lanes move coefficients: they stage the block an AC-refinement lane corrects
// in LDS (it reads every coefficient of its band, and a dependent global load apiece would be the whole run time) and apply the
// 64 bits of a DC-refinement step to 64 blocks.  The scans of one level touch disjoint (component, coefficient) cells of a
// picture, and the segments of one scan disjoint blocks, so no two lanes of a launch write the same int16.
// A unit is one block of the scan in coding order: an interleaved scan walks the padded MCU grid as the baseline scan does; a scan
// of one component covers the ceil(dw / 8) x ceil(dh / 8) blocks that hold its samples in raster order, and that is what its
// restart interval counts.
struct ScanMap {
    bool inter;
    BlockMap bm;
    int c, sw, bwc;
    long basec, units;

    __device__ inline void init(const sat_jpeg_desc& d, const sat_jpeg_scan& sc) {
        inter = sc.n_components > 1;
        bm.init(d);
        c = sc.component[0];
        const CompGeom g = comp_geom(d, c);
        sw = (g.dw + 7) / 8; bwc = g.bw;
        basec = c == 0 ? bm.base0 : (c == 1 ? bm.base1 : bm.base2);
        units = inter ? bm.total : (long)sw * ((g.dh + 7) / 8);
    }
    __device__ inline int per_mcu() const { return inter ? bm.slots : 1; }
    __device__ inline long block(long u) const {
        if (inter) return bm.block(u / bm.slots, (int)(u % bm.slots));
        return basec + (u / sw) * bwc + u % sw;
    }
    __device__ inline int comp(long u) const {
        if (!inter) return c;
        const int slot = (int)(u % bm.slots);
        return slot < bm.ny ? 0 : slot - bm.ny + 1;
    }
};

__host__ __device__ inline long scan_units(const sat_jpeg_desc& d, const sat_jpeg_scan& sc) {
    if (sc.n_components > 1) return picture_mcus(d);
    const CompGeom g = comp_geom(d, sc.component[0]);
    return (long)((g.dw + 7) / 8) * ((g.dh + 7) / 8);
}

__device__ inline int get_bits(BitReader& br, int n) {
    br.refill();
    const int v = (int)br.peek(n);
    br.skip(n);
    return v;
}

// decode_mcu_AC_first, one block
__device__ inline void prog_ac_first(BitReader& br, const sat_jpeg_htable& t, int ss, int se, int al, int& eobrun, int16_t* __restrict__ blk) {
    if (eobrun > 0) { --eobrun; return; }
    for (int k = ss; k <= se; ++k) {
        const int rs = huff_decode(br, t);
        if (rs < 0) return;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > se) { br.flags |= JPEG_BAD_INDEX; return; }
            blk[k_natural_order[k]] = (int16_t)((unsigned)receive_extend(br, s) << al);
        } else if (r == 15) {
            k += 15;
        } else {
            eobrun = 1 << r;
            if (r) eobrun += get_bits(br, r);
            --eobrun;                                             // this block is the first of the run
            return;
        }
    }
}

// a correction bit for a coefficient that is already non-zero: add p1 / m1 only if that bit is not set yet
__device__ inline void prog_correct(BitReader& br, int16_t* c, int p1, int m1) {
    if (get_bits(br, 1)) {
        const int v = *c;
        if ((v & p1) == 0) *c = (int16_t)(v >= 0 ? v + p1 : v + m1);
    }
}

// decode_mcu_AC_refine, one block (in LDS)
__device__ inline void prog_ac_refine(BitReader& br, const sat_jpeg_htable& t, int ss, int se, int al, int& eobrun, int16_t* blk) {
    const int p1 = 1 << al, m1 = -p1;
    int k = ss;
    if (eobrun == 0) {
        for (; k <= se; ++k) {
            const int rs = huff_decode(br, t);
            if (rs < 0) return;
            int r = rs >> 4, s = rs & 15;
            if (s) {
                s = get_bits(br, 1) ? p1 : m1;                    // the size is 1 in a good stream; libjpeg reads one bit whatever it is
            } else if (r != 15) {
                eobrun = 1 << r;
                if (r) eobrun += get_bits(br, r);
                break;                                            // the rest of this block is worked off below
            }
            // pass r zero-valued positions (16 for a ZRL), correcting the non-zero ones on the way
            do {
                int16_t* c = blk + k_natural_order[k];
                if (*c != 0) prog_correct(br, c, p1, m1);
                else if (--r < 0) break;
                ++k;
            } while (k <= se);
            if (s) {
                if (k > se) { br.flags |= JPEG_BAD_INDEX; return; }
                blk[k_natural_order[k]] = (int16_t)s;
            }
            if (br.flags & ~JPEG_MARKER) return;
        }
    }
    if (eobrun > 0) {
        for (; k <= se; ++k) {
            int16_t* c = blk + k_natural_order[k];
            if (*c != 0) prog_correct(br, c, p1, m1);
        }
        --eobrun;
    }
}

__global__ __launch_bounds__(64) void jpeg_prog_entropy_kernel(const uint8_t* __restrict__ comp, long comp_bytes, const sat_jpeg_desc* __restrict__ desc,
                                                               const sat_jpeg_scan* __restrict__ scans, int scan_lo, int scan_hi, int seg_lo,
                                                               const sat_jpeg_htable* __restrict__ huff, int16_t* __restrict__ coefs,
                                                               int* __restrict__ status) {
    __shared__ sat_jpeg_htable tabs[3];
    __shared__ int16_t sblk[64];
    __shared__ uint32_t smask[2];
    const int seg_global = seg_lo + blockIdx.x;
    int lo = scan_lo, hi = scan_hi - 1;                          // scan of this level: last one whose segment_base <= seg_global
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scans[mid].segment_base <= seg_global) lo = mid; else hi = mid - 1;
    }
    const sat_jpeg_scan& sc = scans[lo];
    const int seg = seg_global - sc.segment_base;
    if (seg < 0 || seg >= sc.n_segments) return;
    const int p = sc.picture;
    const sat_jpeg_desc& d = desc[p];
    const int ss = sc.ss, se = sc.se, ah = sc.ah, al = sc.al;
    const bool dc_scan = ss == 0;
    const int nt = dc_scan ? (ah == 0 ? sc.n_components : 0) : 1;          // a DC refinement reads raw bits only
    for (int t = 0; t < nt; ++t) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + (dc_scan ? sc.dc_table[t] : sc.ac_table));
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tabs[t]);
        for (int k = threadIdx.x; k < (int)(sizeof(sat_jpeg_htable) / 4); k += blockDim.x) dst[k] = src[k];
    }
    __syncthreads();
    const int tid = threadIdx.x;
    ScanMap map;
    map.init(d, sc);
    const long ri = (long)sc.restart_interval * map.per_mcu();
    const long u0 = ri ? (long)seg * ri : 0;
    const long u1 = ri ? min(map.units, u0 + ri) : map.units;

    BitReader br;
    br.base = comp; br.abs0 = sc.data_offset; br.pos = 0; br.end = 0; br.limit = comp_bytes;
    br.buf = 0; br.cnt = 0; br.fill = 0; br.flags = 0; br.word_idx = -1; br.word = 0;
    {
        const uint32_t* segtab = reinterpret_cast<const uint32_t*>(comp + sc.segments_offset);
        const long s0 = segtab[2 * seg], s1 = segtab[2 * seg + 1];
        if (s0 > s1 || s1 > sc.data_bytes) {                      // the whole wave leaves: no barrier is left waiting
            if (tid == 0) atomicOr(status + p, JPEG_BAD_SEGMENT);
            return;
        }
        br.pos = s0; br.end = s1;
    }

    if (dc_scan && ah == 0) {                                     // DC first: lane 0 alone
        if (tid != 0) return;
        int dc0 = 0, dc1 = 0, dc2 = 0;                            // the predictors start at 0 in every restart segment
        for (long u = u0; u < u1 && !(br.flags & ~JPEG_MARKER); ++u) {
            const int c = map.comp(u);
            const int slot = map.inter ? c : 0;
            const int s = huff_decode(br, tabs[slot]);
            if (s > 15) br.flags |= JPEG_BAD_CODE;
            if (s >= 0 && s <= 15) {
                const int dcv = (c == 0 ? dc0 : (c == 1 ? dc1 : dc2)) + receive_extend(br, s);
                if (c == 0) dc0 = dcv; else if (c == 1) dc1 = dcv; else dc2 = dcv;
                const int16_t v = (int16_t)((unsigned)dcv << al);
                if (v) coefs[map.block(u) * 64] = v;
            }
            if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
        }
        if (br.flags) atomicOr(status + p, br.flags);
    } else if (dc_scan) {                                         // DC refine: bit i of the segment belongs to unit u0 + i
        const int16_t p1 = (int16_t)(1 << al);
        for (long u = u0; u < u1; u += 64) {
            int bad = 0;
            if (tid == 0) {
                const int nb = (int)min(64L, u1 - u);
                uint32_t m0 = 0, m1 = 0;
                for (int i = 0; i < nb; ++i) {
                    const uint32_t bit = (uint32_t)get_bits(br, 1);
                    if (i < 32) m0 |= bit << i; else m1 |= bit << (i - 32);
                }
                if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
                smask[0] = m0; smask[1] = m1;
                bad = br.flags & ~JPEG_MARKER;
            }
            __syncthreads();
            if (u + tid < u1 && ((smask[tid >> 5] >> (tid & 31)) & 1u)) {
                int16_t* b = coefs + map.block(u + tid) * 64;
                b[0] = (int16_t)(b[0] | p1);
            }
            if (__syncthreads_or(bad)) break;                     // also: smask is free again
        }
        if (tid == 0 && br.flags) atomicOr(status + p, br.flags);
    } else if (ah == 0) {                                         // AC first: lane 0 alone, only the non-zero coefficients are stored
        if (tid != 0) return;
        int eobrun = 0;                                           // and so does EOBRUN
        for (long u = u0; u < u1 && !(br.flags & ~JPEG_MARKER); ++u) {
            if (eobrun > 0) { --eobrun; continue; }
            prog_ac_first(br, tabs[0], ss, se, al, eobrun, coefs + map.block(u) * 64);
            if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
        }
        if (br.flags) atomicOr(status + p, br.flags);
    } else {                                                      // AC refine: the block goes through LDS
        int eobrun = 0;
        int16_t next = u0 < u1 ? coefs[map.block(u0) * 64 + tid] : (int16_t)0;
        for (long u = u0; u < u1; ++u) {
            int16_t* blk = coefs + map.block(u) * 64;
            const int16_t v = next;
            sblk[tid] = v;
            if (u + 1 < u1) next = coefs[map.block(u + 1) * 64 + tid];        // in flight while lane 0 decodes this block
            __syncthreads();
            int bad = 0;
            if (tid == 0) {
                prog_ac_refine(br, tabs[0], ss, se, al, eobrun, sblk);
                if (br.overrun()) br.flags |= JPEG_OUT_OF_DATA;
                bad = br.flags & ~JPEG_MARKER;
            }
            const int stop = __syncthreads_or(bad);
            const int16_t w = sblk[tid];
            if (w != v) blk[tid] = w;
            if (stop) break;
        }
        if (tid == 0 && br.flags) atomicOr(status + p, br.flags);
    }
}

// info rows of the progressive pictures: (3, scans, levels, 0)
__global__ __launch_bounds__(256) void jpeg_prog_info_kernel(const sat_jpeg_scan* __restrict__ scans, int n_scans, int n, int* __restrict__ info) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int cnt = 0, top = -1;
    for (int i = 0; i < n_scans; ++i)
        if (scans[i].picture == p) { ++cnt; top = max(top, scans[i].level); }
    info[4 * p] = 3; info[4 * p + 1] = cnt; info[4 * p + 2] = top + 1; info[4 * p + 3] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- 2. IDCT
// jidctint.c, CONST_BITS 13, PASS1_BITS 2; JLONG arithmetic (64-bit) and an int workspace, as libjpeg on LP64.
constexpr int CB = 13, P1 = 2;
constexpr long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
               F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

__device__ inline long descale(long x, int n) { return (x + (1L << (n - 1))) >> n; }

// one 1-D pass: in[0..7] -> out[0..7] descaled by `sh`
template <typename T>
__device__ inline void idct_1d(const T* in, long* out, int sh) {
    long z2 = in[2], z3 = in[6];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847);
    long tmp3 = z1 + z2 * F0_765;
    z2 = in[0]; z3 = in[4];
    long tmp0 = (z2 + z3) << CB;
    long tmp1 = (z2 - z3) << CB;
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298; tmp1 *= F2_053; tmp2 *= F3_072; tmp3 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, sh); out[7] = descale(tmp10 - tmp3, sh);
    out[1] = descale(tmp11 + tmp2, sh); out[6] = descale(tmp11 - tmp2, sh);
    out[2] = descale(tmp12 + tmp1, sh); out[5] = descale(tmp12 - tmp1, sh);
    out[3] = descale(tmp13 + tmp0, sh); out[4] = descale(tmp13 - tmp0, sh);
}

// IDCT_range_limit(cinfo)[x & RANGE_MASK] (jdmaster.c prepare_range_limit_table): x in [-128, 127] -> x + 128; the rest of
// [128, 511] -> 255, of [512, 895] -> 0; [896, 1023] (x < -128 read modulo 1024) -> x - 896
__device__ inline uint8_t range_limit(long x) {
    const int y = (int)x & 1023;
    if (y < 128) return (uint8_t)(y + 128);
    if (y < 512) return 255;
    if (y < 896) return 0;
    return (uint8_t)(y - 896);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const sat_jpeg_desc* __restrict__ desc, const sat_jpeg_qtable* __restrict__ quant,
                                                        const int16_t* __restrict__ coefs, uint8_t* __restrict__ planes) {
    const sat_jpeg_desc& d = desc[blockIdx.y];
    const CompGeom g0 = comp_geom(d, 0), g1 = comp_geom(d, d.components - 1);          // g1: both chroma components
    const long nb0 = (long)g0.bw * g0.bh, nb1 = d.components == 3 ? (long)g1.bw * g1.bh : 0;
    const long total = nb0 + 2 * nb1;
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < total; b += (long)gridDim.x * blockDim.x) {
        const int c = b < nb0 ? 0 : (b < nb0 + nb1 ? 1 : 2);
        const long lb = c == 0 ? b : (c == 1 ? b - nb0 : b - nb0 - nb1);
        const int bw = c == 0 ? g0.bw : g1.bw;
        const uint16_t* q = quant[d.quant[c]].q;
        const long gb = d.block_offset + b;
        int16_t in[64];
#pragma unroll
        for (int k = 0; k < 8; ++k) reinterpret_cast<uint4*>(in)[k] = reinterpret_cast<const uint4*>(coefs + gb * 64)[k];
        int ws[64];
#pragma unroll
        for (int col = 0; col < 8; ++col) {                  // pass 1: columns, into the int workspace
            long x[8], y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = (long)in[8 * k + col] * (long)q[8 * k + col];
            idct_1d(x, y, CB - P1);
#pragma unroll
            for (int k = 0; k < 8; ++k) ws[8 * k + col] = (int)y[k];
        }
        const long row0 = (lb / bw) * 8, col0 = (lb % bw) * 8;
        uint8_t* out = planes + gb * 64 - lb * 64 + row0 * (bw * 8) + col0;      // the component's plane starts at its first block * 64
#pragma unroll
        for (int r = 0; r < 8; ++r) {                        // pass 2: rows
            long y[8];
            idct_1d(ws + 8 * r, y, CB + P1 + 3);
            uint64_t v = 0;
            for (int k = 0; k < 8; ++k) v |= (uint64_t)range_limit((long)(int)y[k]) << (8 * k);
            *reinterpret_cast<uint64_t*>(out + (long)r * bw * 8) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- 3. colour
__device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the component's sample at output pixel (x, y) after jdsample.c's upsampling
__device__ inline int upsampled(const uint8_t* P, const CompGeom& g, int hmax, int vmax, int x, int y) {
    const int pw = g.bw * 8;
    if (g.hs == hmax && g.vs == vmax) return P[(long)y * pw + x];                     // fullsize
    const int i = x >> 1;
    if (g.dw <= 2) return P[(long)(vmax == 2 ? y >> 1 : y) * pw + i];                   // h2v1_upsample / h2v2_upsample
    if (vmax == 1) {                                                                  // h2v1_fancy_upsample
        const uint8_t* row = P + (long)y * pw;
        const int s = 3 * row[i];
        return (x & 1) ? (s + row[min(i + 1, g.dw - 1)] + 2) >> 2 : (s + row[max(i - 1, 0)] + 1) >> 2;
    }
    const int j = y >> 1;                                                             // h2v2_fancy_upsample
    const int jf = (y & 1) ? min(j + 1, g.dh - 1) : max(j - 1, 0);
    const uint8_t* near = P + (long)j * pw;
    const uint8_t* far = P + (long)jf * pw;
    const int cs = 3 * near[i] + far[i];
    if (x & 1) {
        const int k = min(i + 1, g.dw - 1);
        return (3 * cs + 3 * near[k] + far[k] + 7) >> 4;
    }
    const int k = max(i - 1, 0);
    return (3 * cs + 3 * near[k] + far[k] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const sat_jpeg_desc* __restrict__ desc, const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ pixels) {
    const sat_jpeg_desc d = desc[blockIdx.y];
    CompGeom g[3];
    const uint8_t* P[3];
    long base = d.block_offset * 64;
    for (int c = 0; c < d.components; ++c) { g[c] = comp_geom(d, c); P[c] = planes + base; base += (long)g[c].bw * g[c].bh * 64; }
    const int hmax = d.components == 3 ? d.h_samp : 1, vmax = d.components == 3 ? d.v_samp : 1;
    const long npx = (long)d.height * d.width;
    uint8_t* out = pixels + d.out_offset;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < npx; t += (long)gridDim.x * blockDim.x) {
        const int y = (int)(t / d.width), x = (int)(t % d.width);
        const int Y = P[0][(long)y * (g[0].bw * 8) + x];
        int r = Y, gg = Y, b = Y;
        if (d.components == 3) {
            const int cb = upsampled(P[1], g[1], hmax, vmax, x, y) - 128, cr = upsampled(P[2], g[2], hmax, vmax, x, y) - 128;
            // jdcolor.c build_ycc_rgb_table, SCALEBITS 16: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802,
            // FIX(0.34414) = 22554, ONE_HALF = 32768
            r = clamp255(Y + ((91881 * cr + 32768) >> 16));
            gg = clamp255(Y + ((-46802 * cr + (-22554 * cb + 32768)) >> 16));
            b = clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
        out[3 * t] = (uint8_t)r; out[3 * t + 1] = (uint8_t)gg; out[3 * t + 2] = (uint8_t)b;
    }
}

int validate(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* dh, const sat_jpeg_desc* dd, int32_t n, const void* quant,
             int32_t n_quant, const void* huff, int32_t n_huff, const uint8_t* pixels, int64_t pixels_bytes, const int32_t* status,
             long* blocks_out, long* segs_out, long* max_px, long* max_blocks) {
    SAT_REQUIRE(dh && dd && n > 0 && n <= 65535, "sat_jpeg_decode_batch: null descriptors or n = %d (1 ... 65535)", n);
    SAT_REQUIRE(compressed && compressed_bytes > 0 && quant && n_quant > 0 && huff && n_huff > 0 && pixels && pixels_bytes > 0 && status,
                "sat_jpeg_decode_batch: null buffer or empty table array");
    long blocks = 0, segs = 0;
    *max_px = *max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const sat_jpeg_desc& d = dh[i];
        SAT_REQUIRE(d.height >= 1 && d.height <= 65535 && d.width >= 1 && d.width <= 65535, "jpeg %d: size %dx%d", i, d.height, d.width);
        SAT_REQUIRE(d.components == 1 || d.components == 3, "jpeg %d: %d components (1 or 3)", i, d.components);
        if (d.components == 3)
            SAT_REQUIRE((d.h_samp == 1 && d.v_samp == 1) || (d.h_samp == 2 && d.v_samp == 1) || (d.h_samp == 2 && d.v_samp == 2),
                        "jpeg %d: luma sampling %dx%d (1x1, 2x1 or 2x2)", i, d.h_samp, d.v_samp);
        else
            SAT_REQUIRE(d.h_samp == 1 && d.v_samp == 1, "jpeg %d: a grayscale picture takes sampling 1x1", i);
        SAT_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "jpeg %d: restart interval %d", i, d.restart_interval);
        const long mcus = picture_mcus(d);
        const long want = d.restart_interval ? (mcus + d.restart_interval - 1) / d.restart_interval : 1;
        SAT_REQUIRE(d.n_segments == want, "jpeg %d: %d segments, the restart interval makes %ld", i, d.n_segments, want);
        SAT_REQUIRE(d.segment_base == segs, "jpeg %d: segment_base %d, expected %ld", i, d.segment_base, segs);
        SAT_REQUIRE(d.block_offset == blocks, "jpeg %d: block_offset %ld, expected %ld", i, (long)d.block_offset, blocks);
        SAT_REQUIRE(d.data_offset >= 0 && d.data_bytes >= 0 && d.data_offset + d.data_bytes <= compressed_bytes, "jpeg %d: data outside the buffer", i);
        SAT_REQUIRE(d.segments_offset >= 0 && d.segments_offset % 4 == 0 && d.segments_offset + 8L * d.n_segments <= compressed_bytes,
                    "jpeg %d: segment table outside the buffer or not 4-byte aligned", i);
        SAT_REQUIRE(d.out_offset >= 0 && d.out_offset + 3L * d.height * d.width <= pixels_bytes, "jpeg %d: output outside the pixel buffer", i);
        for (int c = 0; c < 3; ++c)
            SAT_REQUIRE(d.quant[c] >= 0 && d.quant[c] < n_quant && d.dc_table[c] >= 0 && d.dc_table[c] < n_huff && d.ac_table[c] >= 0 &&
                            d.ac_table[c] < n_huff, "jpeg %d: table index out of range", i);
        const long nb = picture_blocks(d);
        blocks += nb;
        segs += d.n_segments;
        SAT_REQUIRE(segs < (1L << 31), "sat_jpeg_decode_batch: too many segments");
        if (nb > *max_blocks) *max_blocks = nb;
        if ((long)d.height * d.width > *max_px) *max_px = (long)d.height * d.width;
    }
    *blocks_out = blocks;
    *segs_out = segs;
    return SAT_OK;
}

// the options of a call: the defaults filled in, checked
struct ParOpts { int subseq; long min_bytes; int32_t* info; };

int par_opts(const sat_jpeg_decode_opts* o, const char* who, ParOpts* out) {
    out->subseq = SAT_JPEG_SUBSEQ_BYTES_DEFAULT; out->min_bytes = SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT; out->info = nullptr;
    if (!o) return SAT_OK;
    SAT_REQUIRE(o->subseq_bytes == 0 || (o->subseq_bytes >= 16 && o->subseq_bytes % 4 == 0 && o->subseq_bytes <= (1 << 20)),
                "%s: subseq_bytes = %d (0 for the default, else a multiple of 4 from 16 to 2^20)", who, o->subseq_bytes);
    SAT_REQUIRE(o->parallel_min_bytes >= -1, "%s: parallel_min_bytes = %lld (-1 for the default, else >= 0)", who, (long long)o->parallel_min_bytes);
    if (o->subseq_bytes) out->subseq = o->subseq_bytes;
    if (o->parallel_min_bytes >= 0) out->min_bytes = o->parallel_min_bytes;
    out->info = o->info;
    return SAT_OK;
}

// subsequences of the pictures the parallel path may take (all of them, and the most of one picture)
void par_count(const sat_jpeg_desc* dh, int n, const ParOpts& o, long* subs, long* max_subs) {
    *subs = *max_subs = 0;
    for (int i = 0; i < n; ++i) {
        if (!par_takes(dh[i], o.min_bytes)) continue;
        const long ns = (dh[i].data_bytes + o.subseq - 1) / o.subseq;
        *subs += ns;
        if (ns > *max_subs) *max_subs = ns;
    }
}

// workspace: coefficients | sample planes | control words | exit states | entry states | blocks completed | first block
size_t par_state_offset(long blocks) { return ((size_t)blocks * (64 * sizeof(int16_t) + 64) + 15) / 16 * 16; }
size_t workspace_need(long blocks, int n, long subs) {
    return par_state_offset(blocks) + (size_t)n * PAR_CTRL * sizeof(int) + (size_t)subs * (2 * sizeof(uint64_t) + 2 * sizeof(int));
}

// the geometry checks both entry points make of a picture
int check_geometry(const sat_jpeg_desc& d, int i) {
    SAT_REQUIRE(d.height >= 1 && d.height <= 65535 && d.width >= 1 && d.width <= 65535, "jpeg %d: size %dx%d", i, d.height, d.width);
    SAT_REQUIRE(d.components == 1 || d.components == 3, "jpeg %d: %d components (1 or 3)", i, d.components);
    if (d.components == 3)
        SAT_REQUIRE((d.h_samp == 1 && d.v_samp == 1) || (d.h_samp == 2 && d.v_samp == 1) || (d.h_samp == 2 && d.v_samp == 2),
                    "jpeg %d: luma sampling %dx%d (1x1, 2x1 or 2x2)", i, d.h_samp, d.v_samp);
    else
        SAT_REQUIRE(d.h_samp == 1 && d.v_samp == 1, "jpeg %d: a grayscale picture takes sampling 1x1", i);
    return SAT_OK;
}

int prog_validate(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* dh, const sat_jpeg_desc* dd, int32_t n,
                  const sat_jpeg_scan* sh, const sat_jpeg_scan* sd, int32_t n_scans, const void* quant, int32_t n_quant, const void* huff,
                  int32_t n_huff, const uint8_t* pixels, int64_t pixels_bytes, const int32_t* status, long* blocks_out, long* max_px, long* max_blocks) {
    const char* who = "sat_jpeg_decode_progressive_batch";
    SAT_REQUIRE(dh && dd && n > 0 && n <= 65535, "%s: null descriptors or n = %d (1 ... 65535)", who, n);
    SAT_REQUIRE(sh && sd && n_scans > 0, "%s: null scan records or n_scans = %d", who, n_scans);
    SAT_REQUIRE(compressed && compressed_bytes > 0 && quant && n_quant > 0 && huff && n_huff > 0 && pixels && pixels_bytes > 0 && status,
                "%s: null buffer or empty table array", who);
    long blocks = 0;
    *max_px = *max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const sat_jpeg_desc& d = dh[i];
        SAT_TRY(check_geometry(d, i));
        SAT_REQUIRE(d.block_offset == blocks, "jpeg %d: block_offset %ld, expected %ld", i, (long)d.block_offset, blocks);
        SAT_REQUIRE(d.out_offset >= 0 && d.out_offset + 3L * d.height * d.width <= pixels_bytes, "jpeg %d: output outside the pixel buffer", i);
        for (int c = 0; c < 3; ++c) SAT_REQUIRE(d.quant[c] >= 0 && d.quant[c] < n_quant, "jpeg %d: table index out of range", i);
        const long nb = picture_blocks(d);
        blocks += nb;
        if (nb > *max_blocks) *max_blocks = nb;
        if ((long)d.height * d.width > *max_px) *max_px = (long)d.height * d.width;
    }
    long segs = 0;
    int level = 0;
    for (int i = 0; i < n_scans; ++i) {
        const sat_jpeg_scan& sc = sh[i];
        SAT_REQUIRE(sc.picture >= 0 && sc.picture < n, "scan %d: picture %d of %d", i, sc.picture, n);
        const sat_jpeg_desc& d = dh[sc.picture];
        SAT_REQUIRE(sc.level >= level, "scan %d: level %d behind level %d (the records are ordered by level)", i, sc.level, level);
        level = sc.level;
        SAT_REQUIRE((sc.n_components == 1 && sc.component[0] >= 0 && sc.component[0] < d.components) ||
                        (sc.n_components == 3 && d.components == 3 && sc.component[0] == 0 && sc.component[1] == 1 && sc.component[2] == 2),
                    "scan %d: components (one, or all three in order)", i);
        if (sc.ss == 0)
            SAT_REQUIRE(sc.se == 0, "scan %d: band %d..%d mixes DC and AC", i, sc.ss, sc.se);
        else
            SAT_REQUIRE(sc.n_components == 1 && sc.ss >= 1 && sc.ss <= sc.se && sc.se <= 63, "scan %d: AC band %d..%d of %d components", i, sc.ss, sc.se,
                        sc.n_components);
        SAT_REQUIRE(sc.ah >= 0 && sc.ah <= 13 && sc.al >= 0 && sc.al <= 13 && (sc.ah == 0 || sc.al == sc.ah - 1),
                    "scan %d: successive approximation Ah %d Al %d", i, sc.ah, sc.al);
        if (sc.ss == 0 && sc.ah == 0)
            for (int c = 0; c < sc.n_components; ++c)
                SAT_REQUIRE(sc.dc_table[c] >= 0 && sc.dc_table[c] < n_huff, "scan %d: table index out of range", i);
        if (sc.ss) SAT_REQUIRE(sc.ac_table >= 0 && sc.ac_table < n_huff, "scan %d: table index out of range", i);
        SAT_REQUIRE(sc.restart_interval >= 0 && sc.restart_interval <= 65535, "scan %d: restart interval %d", i, sc.restart_interval);
        const long units = scan_units(d, sc);
        const long want = sc.restart_interval ? (units + sc.restart_interval - 1) / sc.restart_interval : 1;
        SAT_REQUIRE(sc.n_segments == want, "scan %d: %d segments, the restart interval makes %ld", i, sc.n_segments, want);
        SAT_REQUIRE(sc.segment_base == segs, "scan %d: segment_base %d, expected %ld", i, sc.segment_base, segs);
        SAT_REQUIRE(sc.data_offset >= 0 && sc.data_bytes >= 0 && sc.data_offset + sc.data_bytes <= compressed_bytes, "scan %d: data outside the buffer", i);
        SAT_REQUIRE(sc.segments_offset >= 0 && sc.segments_offset % 4 == 0 && sc.segments_offset + 8L * sc.n_segments <= compressed_bytes,
                    "scan %d: segment table outside the buffer or not 4-byte aligned", i);
        segs += sc.n_segments;
        SAT_REQUIRE(segs < (1L << 31), "%s: too many segments", who);
    }
    *blocks_out = blocks;
    return SAT_OK;
}

}  // namespace
}  // namespace sat

using namespace sat;

extern "C" {

size_t sat_jpeg_decode_workspace_bytes_ex(const sat_jpeg_desc* desc_host, int32_t n, const sat_jpeg_decode_opts* opts) {
    if (!desc_host || n <= 0) { fail(SAT_EINVAL, "sat_jpeg_decode_workspace_bytes: null descriptors or n = %d", n); return 0; }
    ParOpts o;
    if (par_opts(opts, "sat_jpeg_decode_workspace_bytes", &o) != SAT_OK) return 0;
    long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const sat_jpeg_desc& d = desc_host[i];
        if (d.height < 1 || d.width < 1 || !(d.components == 1 || d.components == 3) || d.h_samp < 1 || d.h_samp > 2 || d.v_samp < 1 ||
            d.v_samp > 2) {
            fail(SAT_EINVAL, "sat_jpeg_decode_workspace_bytes: jpeg %d has a bad geometry", i);
            return 0;
        }
        blocks += picture_blocks(d);
    }
    long subs = 0, max_subs = 0;
    par_count(desc_host, n, o, &subs, &max_subs);
    return workspace_need(blocks, n, subs);
}

size_t sat_jpeg_decode_workspace_bytes(const sat_jpeg_desc* desc_host, int32_t n) { return sat_jpeg_decode_workspace_bytes_ex(desc_host, n, nullptr); }

int sat_jpeg_decode_batch_ex(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host, const sat_jpeg_desc* desc_dev,
                             int32_t n, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev, int32_t n_huff,
                             uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream,
                             const sat_jpeg_decode_opts* opts) {
    ParOpts o;
    SAT_TRY(par_opts(opts, "sat_jpeg_decode_batch", &o));
    long blocks = 0, segs = 0, max_px = 0, max_blocks = 0;
    SAT_TRY(validate(compressed, compressed_bytes, desc_host, desc_dev, n, quant_dev, n_quant, huff_dev, n_huff, pixels, pixels_bytes, status,
                     &blocks, &segs, &max_px, &max_blocks));
    long subs = 0, max_subs = 0;
    par_count(desc_host, n, o, &subs, &max_subs);
    SAT_REQUIRE(subs < (1L << 31), "sat_jpeg_decode_batch: %ld subsequences (raise subseq_bytes)", subs);
    const size_t need = workspace_need(blocks, n, subs);
    SAT_REQUIRE(workspace && workspace_bytes >= need, "sat_jpeg_decode_batch: workspace %zu bytes, need %zu", workspace_bytes, need);
    SAT_REQUIRE(((uintptr_t)compressed & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0 && ((uintptr_t)status & 3) == 0 &&
                    ((uintptr_t)huff_dev & 3) == 0 && ((uintptr_t)quant_dev & 1) == 0 && ((uintptr_t)o.info & 3) == 0,
                "sat_jpeg_decode_batch: compressed (4), workspace (16), records (8), status, info and tables must be aligned");
    hipStream_t st = (hipStream_t)stream;
    int16_t* coefs = reinterpret_cast<int16_t*>(workspace);
    uint8_t* planes = reinterpret_cast<uint8_t*>(workspace) + (size_t)blocks * 64 * sizeof(int16_t);
    int* ctrl = reinterpret_cast<int*>(reinterpret_cast<uint8_t*>(workspace) + par_state_offset(blocks));
    uint64_t* st_exit = reinterpret_cast<uint64_t*>(ctrl + (size_t)n * PAR_CTRL);          // n * 32 bytes behind a 16-byte boundary: 8-byte aligned
    uint64_t* st_entry = st_exit + subs;
    int* nblk = reinterpret_cast<int*>(st_entry + subs);
    int* blk_base = nblk + subs;
    int* stat = reinterpret_cast<int*>(status);
    const long cbytes = (long)compressed_bytes;
    SAT_TRY(dev_fill_bytes(st, status, 0, sizeof(int32_t) * (size_t)n));
    SAT_TRY(dev_fill_bytes(st, coefs, 0, (size_t)blocks * 64 * sizeof(int16_t)));
    if (subs == 0) {                                            // today's path: every picture on the serial lanes
        if (o.info) SAT_TRY(dev_fill_bytes(st, o.info, 0, 4 * sizeof(int32_t) * (size_t)n));
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)segs), dim3(64), 0, st, compressed, cbytes, desc_dev, n, huff_dev, coefs, stat,
                           (const int*)nullptr);
        SAT_TRY(launch_ok("jpeg_entropy_kernel"));
    } else {
        const dim3 lanes((unsigned)min(cdiv(max_subs, PAR_THREADS), 4096), (unsigned)n);
        hipLaunchKernelGGL(jpeg_par_setup_kernel, dim3(1), dim3(PAR_THREADS), 0, st, compressed, cbytes, desc_dev, n, o.subseq, o.min_bytes, subs, ctrl);
        SAT_TRY(launch_ok("jpeg_par_setup_kernel"));
        hipLaunchKernelGGL(jpeg_par_spec_kernel, lanes, dim3(PAR_THREADS), 0, st, compressed, cbytes, desc_dev, huff_dev, o.subseq, ctrl, st_exit, st_entry,
                           nblk);
        SAT_TRY(launch_ok("jpeg_par_spec_kernel"));
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)segs), dim3(64), 0, st, compressed, cbytes, desc_dev, n, huff_dev, coefs, stat,
                           (const int*)ctrl);
        SAT_TRY(launch_ok("jpeg_entropy_kernel"));
        hipLaunchKernelGGL(jpeg_par_sync_kernel, dim3((unsigned)n), dim3(PAR_SYNC_THREADS), 0, st, compressed, cbytes, desc_dev, huff_dev, o.subseq, ctrl,
                           st_exit, st_entry, nblk, blk_base);
        SAT_TRY(launch_ok("jpeg_par_sync_kernel"));
        hipLaunchKernelGGL(jpeg_par_write_kernel, lanes, dim3(PAR_THREADS), 0, st, compressed, cbytes, desc_dev, huff_dev, o.subseq, ctrl,
                           (const uint64_t*)st_exit, (const uint64_t*)st_entry, (const int*)blk_base, coefs);
        SAT_TRY(launch_ok("jpeg_par_write_kernel"));
        hipLaunchKernelGGL(jpeg_par_dc_kernel, dim3(3, (unsigned)n), dim3(PAR_THREADS), 0, st, desc_dev, (const int*)ctrl, coefs);
        SAT_TRY(launch_ok("jpeg_par_dc_kernel"));
        hipLaunchKernelGGL(jpeg_par_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, compressed, cbytes, desc_dev, huff_dev, (const int*)ctrl, coefs, stat,
                           reinterpret_cast<int*>(o.info));
        SAT_TRY(launch_ok("jpeg_par_finish_kernel"));
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)min(cdiv(max_blocks, 256), 1024), (unsigned)n), dim3(256), 0, st, desc_dev, quant_dev, coefs,
                       planes);
    SAT_TRY(launch_ok("jpeg_idct_kernel"));
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)min(cdiv(max_px, 256), 1024), (unsigned)n), dim3(256), 0, st, desc_dev, planes, pixels);
    SAT_TRY(launch_ok("jpeg_color_kernel"));
    return SAT_OK;
}

int sat_jpeg_decode_batch(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host, const sat_jpeg_desc* desc_dev,
                          int32_t n, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev, int32_t n_huff,
                          uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return sat_jpeg_decode_batch_ex(compressed, compressed_bytes, desc_host, desc_dev, n, quant_dev, n_quant, huff_dev, n_huff, pixels, pixels_bytes,
                                    status, workspace, workspace_bytes, stream, nullptr);
}

size_t sat_jpeg_progressive_workspace_bytes(const sat_jpeg_desc* desc_host, int32_t n, const sat_jpeg_scan* scans_host, int32_t n_scans) {
    if (!desc_host || n <= 0 || !scans_host || n_scans <= 0) {
        fail(SAT_EINVAL, "sat_jpeg_progressive_workspace_bytes: null records, n = %d or n_scans = %d", n, n_scans);
        return 0;
    }
    long blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (check_geometry(desc_host[i], i) != SAT_OK) return 0;
        blocks += picture_blocks(desc_host[i]);
    }
    return par_state_offset(blocks);                           // coefficients | sample planes
}

int sat_jpeg_decode_progressive_batch(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host,
                                      const sat_jpeg_desc* desc_dev, int32_t n, const sat_jpeg_scan* scans_host, const sat_jpeg_scan* scans_dev,
                                      int32_t n_scans, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev,
                                      int32_t n_huff, uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace,
                                      size_t workspace_bytes, void* stream, int32_t* info) {
    long blocks = 0, max_px = 0, max_blocks = 0;
    SAT_TRY(prog_validate(compressed, compressed_bytes, desc_host, desc_dev, n, scans_host, scans_dev, n_scans, quant_dev, n_quant, huff_dev, n_huff,
                          pixels, pixels_bytes, status, &blocks, &max_px, &max_blocks));
    const size_t need = par_state_offset(blocks);
    SAT_REQUIRE(workspace && workspace_bytes >= need, "sat_jpeg_decode_progressive_batch: workspace %zu bytes, need %zu", workspace_bytes, need);
    SAT_REQUIRE(((uintptr_t)compressed & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0 && ((uintptr_t)scans_dev & 7) == 0 &&
                    ((uintptr_t)status & 3) == 0 && ((uintptr_t)huff_dev & 3) == 0 && ((uintptr_t)quant_dev & 1) == 0 && ((uintptr_t)info & 3) == 0,
                "sat_jpeg_decode_progressive_batch: compressed (4), workspace (16), records (8), status, info and tables must be aligned");
    hipStream_t st = (hipStream_t)stream;
    int16_t* coefs = reinterpret_cast<int16_t*>(workspace);
    uint8_t* planes = reinterpret_cast<uint8_t*>(workspace) + (size_t)blocks * 64 * sizeof(int16_t);
    SAT_TRY(dev_fill_bytes(st, status, 0, sizeof(int32_t) * (size_t)n));
    SAT_TRY(dev_fill_bytes(st, coefs, 0, (size_t)blocks * 64 * sizeof(int16_t)));
    if (info) {
        hipLaunchKernelGGL(jpeg_prog_info_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, scans_dev, n_scans, n, reinterpret_cast<int*>(info));
        SAT_TRY(launch_ok("jpeg_prog_info_kernel"));
    }
    // one launch per level: the records are ordered by level, so a level is a run of records and of segments
    for (int lo = 0; lo < n_scans;) {
        int hi = lo;
        long segs = 0;
        while (hi < n_scans && scans_host[hi].level == scans_host[lo].level) segs += scans_host[hi++].n_segments;
        hipLaunchKernelGGL(jpeg_prog_entropy_kernel, dim3((unsigned)segs), dim3(64), 0, st, compressed, (long)compressed_bytes, desc_dev, scans_dev, lo, hi,
                           scans_host[lo].segment_base, huff_dev, coefs, reinterpret_cast<int*>(status));
        SAT_TRY(launch_ok("jpeg_prog_entropy_kernel"));
        lo = hi;
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)min(cdiv(max_blocks, 256), 1024), (unsigned)n), dim3(256), 0, st, desc_dev, quant_dev, coefs,
                       planes);
    SAT_TRY(launch_ok("jpeg_idct_kernel"));
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)min(cdiv(max_px, 256), 1024), (unsigned)n), dim3(256), 0, st, desc_dev, planes, pixels);
    SAT_TRY(launch_ok("jpeg_color_kernel"));
    return SAT_OK;
}

}  // extern "C"
