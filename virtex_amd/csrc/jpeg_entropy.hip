// Huffman decoding of JPEG scans ON THE DEVICE: the stage jpeg.hip leaves to host
// threads.  A Huffman stream has no random access, but it is SELF-SYNCHRONISING: a decoder started at a wrong bit position or in
// a wrong state falls into step with the true decoder after a few code words.  Weissenberger & Schmidt ("Massively Parallel
// Huffman Decoding on GPUs", ICPP 2018) build a parallel decoder on that; this file adapts it to JPEG's block structure.
//
//   layout   the entropy-coded bytes of a restart interval ("segment"; a stream without restart markers is one segment) are cut
//            into subsequences of `subseq_bits` bits, ONE LANE EACH.  The subsequences of all images of a chunk lie side by
//            side; every image is padded to whole workgroups of 256 lanes, so a workgroup serves one image and keeps that
//            image's Huffman tables (1.4 KB each, six at the most) in LDS.
//   state    what a decoder needs at a subsequence's first byte: how many bits of it belong to a symbol that began earlier
//            (0..31: a code of <= 16 bits + <= 15 magnitude bits), the block inside the MCU (-> component -> tables) and the
//            zig-zag index.  Packed into one int; -1 = "no state" (an invalid code was met), which only ever equals itself.
//            Bits are counted behind byte stuffing (FF 00 -> FF), so states do not depend on where stuffed bytes fall.
//   sync     lane i owns subsequence i: it decodes it from an ENTRY state to an EXIT state and a count of coefficient slots
//            (a zero run, ZRL and EOB advance the slot count as coefficients do).  The exit of lane i is the entry of lane i + 1.
//            Round 0 starts every lane from the default state (speculation); in every further round a lane whose entry
//            changed decodes again, until no entry changes (one ballot per wave + one LDS word per wave for the vote).  Lane 0
//            of a segment starts from the true state, so after k rounds k lanes are final whatever the bytes are: <= 256
//            rounds, in practice two or three.  This is the paper's "lane i continues through subsequence i + 1 and compares"
//            with the work booked on the owner of the subsequence; decodes and rounds are the same.
//            Across workgroups the same kernel is launched again (pass p): a workgroup takes the exit of its predecessor's last
//            lane (ping-pong array, so a pass reads only what the pass before wrote) and leaves at once if that is what it
//            assumed.  After pass p the first p + 1 workgroups of every image are final; the host issues as many passes as the
//            largest image has workgroups.  No loop waits for another workgroup.
//   place    per image: exclusive prefix sum of the slot counts -> first slot of every subsequence.  A segment must begin at
//            the slot its MCU count says and the image must fill total_blocks * 64 slots, else the status is set.
//   write    every lane decodes once more from its final entry and scatters: slot -> block in scan order -> component plane
//            -> natural order.  DC values are written as differences; every store is checked against the image's extent and the
//            buffer's, and a lane stops at its segment's last slot, so no byte sequence writes out of bounds or runs long.
//   dc       per component an inclusive (segmented: restart intervals) scan of the DC differences in scan order, in int.
//
// The coefficient buffer holds exactly what vtx_jpeg_entropy_decode writes (tests/test_jpeg_entropy_device.py: bit for bit).
#include "vtx_common.h"
#include "jpeg_entropy.h"

namespace {

constexpr int WG = VTX_JPEG_WG, NW = WG / 64;
constexpr int NO_STATE = -1;
constexpr int LIM_OPEN = 0x7fffffff;

__device__ const unsigned char kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ int pack_state(int over, int blk, int zz) { return over | (blk << 5) | (zz << 8); }

// what a workgroup keeps in LDS of its image
struct ImageLds {
    unsigned tab[VTX_JPEG_MAX_TABLES * (sizeof(VtxJpegTable) / 4)];
    VtxJpegDesc d;
    unsigned char zigzag[64];
};
__device__ __forceinline__ const VtxJpegTable& table(const ImageLds& L, int t) {
    return *reinterpret_cast<const VtxJpegTable*>(&L.tab[t * (sizeof(VtxJpegTable) / 4)]);
}

__device__ __forceinline__ void load_image(ImageLds& L, const unsigned char* __restrict__ chunk, int desc_off) {
    const unsigned* src = reinterpret_cast<const unsigned*>(chunk + desc_off);
    unsigned* dd = reinterpret_cast<unsigned*>(&L.d);
    for (int i = threadIdx.x; i < (int)(sizeof(VtxJpegDesc) / 4); i += WG) dd[i] = src[i];
    if (threadIdx.x < 64) L.zigzag[threadIdx.x] = kZigzagDev[threadIdx.x];
    __syncthreads();
    int ntab = L.d.ntab;
    ntab = ntab < 0 ? 0 : (ntab > VTX_JPEG_MAX_TABLES ? VTX_JPEG_MAX_TABLES : ntab);
    const unsigned* ts = reinterpret_cast<const unsigned*>(chunk + desc_off + L.d.tab_off);
    for (int i = threadIdx.x; i < ntab * (int)(sizeof(VtxJpegTable) / 4); i += WG) L.tab[i] = ts[i];
    __syncthreads();
}

// where lane `sub` of the image works: its segment, the bytes of its subsequence
struct SubRange { int seg, seg_begin, seg_end, begin, end; bool seg_start; };
__device__ __forceinline__ SubRange locate(const ImageLds& L, const VtxJpegSegment* __restrict__ segs, int sub) {
    int lo = 0, hi = L.d.nseg - 1;                      // the last segment whose first subsequence is <= sub (empty segments share
    while (lo < hi) {                                   // a first subsequence with their successor: the LAST one of a tie owns it)
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_sub <= sub) lo = mid; else hi = mid - 1;
    }
    SubRange r;
    r.seg = lo; r.seg_begin = segs[lo].begin; r.seg_end = segs[lo].end;
    const int k = sub - segs[lo].first_sub;
    r.seg_start = k == 0;
    r.begin = r.seg_begin + k * L.d.subseq_bytes;
    r.end = imin(r.begin + L.d.subseq_bytes, r.seg_end);
    return r;
}

// The bit reader of one lane.  `cons` / `loaded` count bits behind byte stuffing from the subsequence's first byte; `lim` is
// the count at which the subsequence ends and `seg_lim` the one at which its segment does (both known as soon as the reader
// tries to load the first byte behind them -- always before `cons` gets there).  Past the segment it feeds zeros.
struct Bits {
    const unsigned char* __restrict__ p;          // the image's scan bytes
    int pos, end, seg_end;
    unsigned long long acc = 0;
    int n = 0, cons = 0, loaded = 0, lim = LIM_OPEN, seg_lim = LIM_OPEN;
    __device__ __forceinline__ void fill() {
        while (n <= 56) {
            if (pos >= end && lim == LIM_OPEN) lim = loaded;
            unsigned b = 0;
            if (pos < seg_end) {
                b = p[pos];
                pos += b == 0xFFu ? 2 : 1;                // inside a segment FF is always followed by its stuffed 00
            } else if (seg_lim == LIM_OPEN) seg_lim = loaded;
            acc |= (unsigned long long)b << (56 - n);
            n += 8; loaded += 8;
        }
    }
    __device__ __forceinline__ int peek(int k) const { return (int)(acc >> (64 - k)); }
    __device__ __forceinline__ void skip(int k) { acc <<= k; n -= k; cons += k; }
    __device__ __forceinline__ int get(int k) { const int v = peek(k); skip(k); return v; }
};

__device__ __forceinline__ int decode_symbol(Bits& br, const VtxJpegTable& h) {
    const int look = h.look[br.peek(9)];
    if (look) { br.skip(look & 15); return look >> 4; }
    const int code = br.peek(16);
    int l = 10;
    for (; l <= 16; ++l)
        if ((code >> (16 - l)) <= h.maxcode[l]) break;
    if (l > 16) return -1;
    br.skip(l);
    return h.vals[((code >> (16 - l)) + h.valptr[l]) & 255];
}
__device__ __forceinline__ int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

struct Decoded { int exit, slots, error; };

// Decode one subsequence from `entry`.  WRITE: scatter the coefficients, beginning at slot `slot0` (image-wide, scan order) and
// stopping at `slot_end`; otherwise only the exit state and the slot count are produced.
template <bool WRITE>
__device__ __forceinline__ Decoded decode_subsequence(const ImageLds& L, const unsigned char* __restrict__ bytes, const SubRange& r,
                                                      int entry, long slot0, long slot_end, short* __restrict__ coef, long coef_room) {
    Decoded out{NO_STATE, 0, 0};
    if (entry == NO_STATE) return out;
    Bits br;
    br.p = bytes; br.end = r.end; br.seg_end = r.seg_end;
    br.pos = r.begin;
    if (r.begin > r.seg_begin && bytes[r.begin - 1] == 0xFFu) ++br.pos;      // the subsequence begins with the 00 of a stuffed pair
    const int bpm = L.d.bpm;
    int blk = (entry >> 5) & 7, zz = entry >> 8;
    int mx = 0, my = 0;
    long slot = slot0, base = 0;
    auto block_base = [&]() {
        const int c = L.d.blk_comp[blk];
        return ((long)L.d.comp_off[c] + (long)(my * L.d.comp_v[c] + L.d.blk_v[blk]) * L.d.comp_bw[c] + mx * L.d.comp_h[c] + L.d.blk_h[blk]) * 64;
    };
    if (WRITE) {
        const long b = slot0 >> 6, mcu = b / bpm;
        blk = (int)(b - mcu * bpm); zz = (int)(slot0 & 63);
        my = (int)(mcu / L.d.mcux); mx = (int)(mcu - (long)my * L.d.mcux);
        base = block_base();
    }
    if (blk >= bpm) return out;
    br.fill();
    br.skip(entry & 31);
    const long room = lmin((long)L.d.total_blocks * 64, coef_room);
    for (;;) {
        br.fill();
        if (br.cons >= br.lim || (WRITE && slot >= slot_end)) break;
        const int comp = L.d.blk_comp[blk], c0 = br.cons;
        int adv = 0, at = zz, val = 0, err = 0;
        bool store = false;
        if (zz == 0) {
            const int t = decode_symbol(br, table(L, L.d.dc_tab[comp]));
            if (t < 0 || t > 11) err = t < 0 ? VTX_JPEG_BAD_CODE : VTX_JPEG_BAD_DC;
            else if (t) { val = extend(br.get(t), t); store = true; }
            adv = 1;
        } else {
            const int rs = decode_symbol(br, table(L, L.d.ac_tab[comp]));
            const int run = rs >> 4, s = rs & 15;
            if (rs < 0) err = VTX_JPEG_BAD_CODE;
            else if (s == 0) adv = run == 15 ? imin(16, 64 - zz) : 64 - zz;    // ZRL / end of block
            else {
                at = zz + run;
                if (at > 63) err = VTX_JPEG_BAD_RUN;
                else { val = extend(br.get(s), s); store = true; adv = run + 1; }
            }
        }
        if (err || br.cons > br.seg_lim) {
            // a symbol that ends behind its segment, or anything in the segment's last (< 8) bits, is padding, not data: the host
            // decoder counts MCUs and never looks at it
            if (br.cons > br.seg_lim || (br.seg_lim != LIM_OPEN && br.seg_lim - c0 < 8)) {
                out.exit = pack_state(0, 0, 0);
                out.slots = (int)(slot - slot0);
            } else out.error = err;
            return out;
        }
        if (WRITE && store) {
            const long idx = base + L.zigzag[at];
            if (idx >= 0 && idx < room) coef[idx] = (short)val;
        }
        zz += adv; slot += adv;
        if (zz >= 64) {
            zz = 0;
            if (++blk == bpm) { blk = 0; if (WRITE && ++mx == L.d.mcux) { mx = 0; ++my; } }
            if (WRITE) base = block_base();
        }
    }
    out.exit = pack_state(imin(br.cons - br.lim, 31), blk, zz);
    out.slots = (int)(slot - slot0);
    return out;
}

// per-chunk scratch, all ints: entry / exit / slots / first slot per lane, the ping-pong exits of the workgroups' last lanes,
// four counters (lanes that were final after 1 / 2 / more decodes of pass 0; decodes of the later passes)
struct Work {
    int* entry; int* exit; int* slots; int* first; int* last[2]; int* stats;
};
__device__ __host__ inline Work carve(int* w, long nwg) {
    Work k;
    const long ns = nwg * WG;
    k.entry = w; k.exit = w + ns; k.slots = w + 2 * ns; k.first = w + 3 * ns;
    k.last[0] = w + 4 * ns; k.last[1] = k.last[0] + nwg; k.stats = k.last[1] + nwg;
    return k;
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(uint4* __restrict__ coef16, long n16, short* __restrict__ tail, int ntail,
                                                          int* __restrict__ status, int nstatus, int* __restrict__ stats) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    for (long k = i; k < n16; k += stride) coef16[k] = make_uint4(0, 0, 0, 0);
    if (i < ntail) tail[i] = 0;
    if (i < nstatus) status[i] = 0;
    if (i < 4) stats[i] = 0;
}

__global__ __launch_bounds__(WG) void jpeg_sync_kernel(const unsigned char* __restrict__ chunk, const int* __restrict__ wg_desc,
                                                       int* __restrict__ workp, int nwg_total, int pass) {
    __shared__ ImageLds L;
    __shared__ int s_exit[WG];
    __shared__ int s_any[NW];
    __shared__ int s_go;
    const int wg = blockIdx.x, l = threadIdx.x, desc_off = wg_desc[wg];
    load_image(L, chunk, desc_off);
    const Work W = carve(workp, nwg_total);
    const int wl = wg - L.d.first_wg;
    if (pass > wl) return;                                // final since pass wl (uniform: the whole workgroup leaves)
    const int sub = wl * WG + l;
    const long g = (long)wg * WG + l;
    const bool active = sub < L.d.nsub;
    const VtxJpegSegment* segs = reinterpret_cast<const VtxJpegSegment*>(chunk + desc_off + L.d.seg_off);
    const unsigned char* bytes = chunk + L.d.byte_off;
    SubRange r{};
    if (active) r = locate(L, segs, sub);
    int entry = 0, exitst = NO_STATE, slots = 0, ndec = 0;
    bool dirty = active;
    if (pass > 0) {
        entry = W.entry[g]; exitst = W.exit[g]; slots = W.slots[g];
        dirty = false;
        if (l == 0) {
            int go = 0;
            if (active && !r.seg_start) {
                const int e = W.last[(pass - 1) & 1][wg - 1];
                if (e != entry) { entry = e; dirty = true; go = 1; }
            }
            s_go = go;
        }
        __syncthreads();
        if (!s_go) {                                      // what the predecessor hands over is what this workgroup assumed
            if (l == WG - 1) W.last[pass & 1][wg] = exitst;
            return;
        }
    }
    for (int round = 0; round <= WG; ++round) {
        if (dirty) {
            const Decoded dcd = decode_subsequence<false>(L, bytes, r, entry, 0, 0, nullptr, 0);
            exitst = dcd.exit; slots = dcd.slots; ++ndec;
        }
        s_exit[l] = exitst;
        __syncthreads();
        const int e = (l > 0 && active && !r.seg_start) ? s_exit[l - 1] : entry;
        dirty = e != entry;
        entry = e;
        const unsigned long long vote = __ballot(dirty);
        if ((l & 63) == 0) s_any[l >> 6] = vote != 0ull;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) any |= s_any[w];
        if (!any) break;
    }
    W.entry[g] = entry; W.exit[g] = exitst; W.slots[g] = slots;
    if (l == WG - 1) W.last[pass & 1][wg] = exitst;
    // statistics: how many decodes a lane needed
    for (int c = 0; c < 4; ++c) {
        const bool mine = active && (pass == 0 ? (c < 3 && imin(ndec, 3) == c + 1) : (c == 3 && ndec > 0));
        const unsigned long long m = __ballot(mine);
        if ((l & 63) == 0 && m) atomicAdd(&W.stats[c], pass == 0 ? __builtin_popcountll(m) : ndec);
    }
}

// one workgroup per image: first slot of every subsequence, and the slot totals the MCU counts ask for
__global__ __launch_bounds__(WG) void jpeg_place_kernel(const unsigned char* __restrict__ chunk, const int* __restrict__ img_desc,
                                                        int* __restrict__ workp, int nwg_total, int* __restrict__ status) {
    __shared__ long long s_scan[WG];
    __shared__ VtxJpegDesc D;
    __shared__ int s_bad;
    const int l = threadIdx.x, desc_off = img_desc[blockIdx.x];
    const unsigned* src = reinterpret_cast<const unsigned*>(chunk + desc_off);
    for (int i = l; i < (int)(sizeof(VtxJpegDesc) / 4); i += WG) reinterpret_cast<unsigned*>(&D)[i] = src[i];
    if (l == 0) s_bad = 0;
    __syncthreads();
    const Work W = carve(workp, nwg_total);
    const long g0 = (long)D.first_wg * WG;
    const long long total_want = (long long)D.total_blocks * 64;
    long long carry = 0;
    for (int base = 0; base < D.nsub; base += WG) {
        const int i = base + l;
        const long long mine = i < D.nsub ? W.slots[g0 + i] : 0;
        long long v = mine;
        s_scan[l] = v;
        __syncthreads();
        for (int d = 1; d < WG; d <<= 1) {
            const long long add = l >= d ? s_scan[l - d] : 0;
            __syncthreads();
            v += add; s_scan[l] = v;
            __syncthreads();
        }
        const long long first = carry + v - mine;
        if (i < D.nsub) W.first[g0 + i] = (int)(first > total_want ? total_want + 1 : first);   // (2^28 pixels at the most: fits)
        carry += s_scan[WG - 1];
        __syncthreads();
    }
    const VtxJpegSegment* segs = reinterpret_cast<const VtxJpegSegment*>(chunk + desc_off + D.seg_off);
    int bad = carry != total_want;
    for (int s = l; s < D.nseg; s += WG) {
        const int fs = segs[s].first_sub;
        const long long have = fs < D.nsub ? (long long)W.first[g0 + fs] : carry;
        if (have != (long long)s * D.seg_mcus * D.bpm * 64) bad = 1;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (l == 0 && s_bad) { status[2 * D.status_slot] = VTX_ERR_ARG; status[2 * D.status_slot + 1] = VTX_JPEG_BAD_TOTAL; }
}

__global__ __launch_bounds__(WG) void jpeg_write_kernel(const unsigned char* __restrict__ chunk, const int* __restrict__ wg_desc,
                                                        const int* __restrict__ workp, int nwg_total, short* __restrict__ coef, long coef_elems,
                                                        int* __restrict__ status) {
    __shared__ ImageLds L;
    const int wg = blockIdx.x, l = threadIdx.x, desc_off = wg_desc[wg];
    load_image(L, chunk, desc_off);
    if (status[2 * L.d.status_slot] != 0) return;        // set by the placement (the launch before): the image stays zero
    const Work W = carve(const_cast<int*>(workp), nwg_total);
    const int sub = (wg - L.d.first_wg) * WG + l;
    if (sub >= L.d.nsub) return;
    const long g = (long)wg * WG + l;
    const VtxJpegSegment* segs = reinterpret_cast<const VtxJpegSegment*>(chunk + desc_off + L.d.seg_off);
    const SubRange r = locate(L, segs, sub);
    const long per_seg = (long)L.d.seg_mcus * L.d.bpm * 64;
    const long slot_end = lmin((long)(r.seg + 1) * per_seg, (long)L.d.total_blocks * 64);
    const long coef_off = (long)(((unsigned long long)(unsigned)L.d.coef_off_hi << 32) | (unsigned)L.d.coef_off_lo);
    if (coef_off < 0 || coef_off >= coef_elems) return;
    const int entry = W.entry[g];
    if (entry == NO_STATE) return;                        // behind an invalid code: the lane that met it reports
    const Decoded dcd = decode_subsequence<true>(L, chunk + L.d.byte_off, r, entry, (long)W.first[g], slot_end, coef + coef_off,
                                                 coef_elems - coef_off);
    if (dcd.error) { status[2 * L.d.status_slot] = VTX_ERR_ARG; status[2 * L.d.status_slot + 1] = dcd.error; }
}

// DC prediction: blockIdx = image * 3 + component; an inclusive scan over the component's blocks in scan order that starts
// again at every restart interval (Hillis-Steele on (value, "a segment head lies at or before me") pairs)
__global__ __launch_bounds__(WG) void jpeg_dc_kernel(const unsigned char* __restrict__ chunk, const int* __restrict__ img_desc,
                                                     short* __restrict__ coef, long coef_elems, const int* __restrict__ status) {
    __shared__ int s_val[WG];
    __shared__ int s_head[WG];
    __shared__ VtxJpegDesc D;
    const int l = threadIdx.x, comp = blockIdx.x % 3, desc_off = img_desc[blockIdx.x / 3];
    const unsigned* src = reinterpret_cast<const unsigned*>(chunk + desc_off);
    for (int i = l; i < (int)(sizeof(VtxJpegDesc) / 4); i += WG) reinterpret_cast<unsigned*>(&D)[i] = src[i];
    __syncthreads();
    if (comp >= D.ncomp || status[2 * D.status_slot] != 0) return;
    const long coef_off = (long)(((unsigned long long)(unsigned)D.coef_off_hi << 32) | (unsigned)D.coef_off_lo);
    const int ch = D.comp_h[comp], cv = D.comp_v[comp], hv = ch * cv, bw = D.comp_bw[comp];
    const long n = (long)D.total_mcus * hv, seg_len = (long)D.seg_mcus * hv;
    const long room = lmin((long)D.total_blocks * 64, coef_elems - coef_off);
    int carry = 0;
    for (long base = 0; base < n; base += WG) {
        const long q = base + l;
        long idx = -1;
        int v = 0, head = 0;
        if (q < n) {
            const long mcu = q / hv;
            const int k = (int)(q - mcu * hv), my = (int)(mcu / D.mcux), mx = (int)(mcu - (long)my * D.mcux);
            idx = ((long)D.comp_off[comp] + (long)(my * cv + k / ch) * bw + mx * ch + k % ch) * 64;
            if (idx < 0 || idx >= room) idx = -1;
            if (idx >= 0) v = coef[coef_off + idx];
            head = q % seg_len == 0;
        }
        s_val[l] = v; s_head[l] = head;
        __syncthreads();
        for (int d = 1; d < WG; d <<= 1) {
            int av = 0, ah = 1;
            if (l >= d) { av = s_val[l - d]; ah = s_head[l - d]; }
            __syncthreads();
            if (l >= d && !head) { v += av; head = ah; }
            s_val[l] = v; s_head[l] = head;
            __syncthreads();
        }
        if (!head) v += carry;
        if (idx >= 0) coef[coef_off + idx] = (short)v;
        s_val[l] = v;
        __syncthreads();
        carry = s_val[WG - 1];
        __syncthreads();
    }
}

}  // namespace

// ---- C ABI ------------------------------------------------------------------------------------------------------------
// chunk_dev: the chunk buffer on the device -- int wg_desc[n_wg] at wg_table_off (per workgroup the byte offset of its image's
// descriptor), int img_desc[n_images] at img_table_off, the descriptors and scan bytes vtx_jpeg_describe wrote.  work_dev:
// (4 * 256 + 2) * n_wg + 4 ints of scratch.  status_dev: 2 ints per image, {0 | VTX_ERR_ARG, reason}.  max_wg: workgroups of the
// largest image (the number of synchronisation passes).  Everything is enqueued on `stream`; nothing is read back.
extern "C" int vtx_jpeg_entropy_decode_device(const void* chunk_dev, long wg_table_off, long img_table_off, int n_images, int n_wg,
                                              int max_wg, short* coef_dev, long coef_elems, int* status_dev, int* work_dev,
                                              long work_ints, void* stream) {
    VTX_CHECK(chunk_dev && coef_dev && status_dev && work_dev, VTX_ERR_ARG, "jpeg_entropy_decode_device: null pointer");
    VTX_CHECK(n_images > 0 && n_wg >= n_images && max_wg >= 1 && max_wg <= n_wg && coef_elems > 0 && wg_table_off >= 0 && img_table_off >= 0 &&
              wg_table_off % 4 == 0 && img_table_off % 4 == 0, VTX_ERR_ARG, "jpeg_entropy_decode_device: bad counts / offsets");
    VTX_CHECK(n_wg <= (1 << 22), VTX_ERR_SHAPE, "jpeg_entropy_decode_device: %d workgroups in one chunk", n_wg);
    VTX_CHECK(work_ints >= (4l * WG + 2) * n_wg + 4, VTX_ERR_WORKSPACE, "jpeg_entropy_decode_device: scratch holds %ld ints, %ld needed",
              work_ints, (4l * WG + 2) * n_wg + 4);
    VTX_CHECK(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)chunk_dev & 15) == 0, VTX_ERR_SHAPE, "jpeg_entropy_decode_device: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* chunk = (const unsigned char*)chunk_dev;
    const int* wg_desc = (const int*)(chunk + wg_table_off);
    const int* img_desc = (const int*)(chunk + img_table_off);
    const Work W = carve(work_dev, n_wg);
    const long n16 = coef_elems / 8;
    const int zero_grid = (int)(n16 / 256 > 4096 ? 4096 : (n16 / 256 < 8 ? 8 : n16 / 256));   // (8 x 256 lanes cover the tail / status / counters)
    VTX_CHECK(2 * n_images <= 8 * 256, VTX_ERR_SHAPE, "jpeg_entropy_decode_device: %d images in one chunk (1024 at the most)", n_images);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, (uint4*)coef_dev, n16, coef_dev + n16 * 8, (int)(coef_elems - n16 * 8),
                       status_dev, 2 * n_images, W.stats);
    for (int pass = 0; pass < max_wg; ++pass)
        hipLaunchKernelGGL(jpeg_sync_kernel, dim3(n_wg), dim3(WG), 0, st, chunk, wg_desc, work_dev, n_wg, pass);
    hipLaunchKernelGGL(jpeg_place_kernel, dim3(n_images), dim3(WG), 0, st, chunk, img_desc, work_dev, n_wg, status_dev);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3(n_wg), dim3(WG), 0, st, chunk, wg_desc, (const int*)work_dev, n_wg, coef_dev, coef_elems, status_dev);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3 * n_images), dim3(WG), 0, st, chunk, img_desc, coef_dev, coef_elems, (const int*)status_dev);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
