// Grouped 3x3 / pad-1 convolutions (stride 1 or 2) on NHWC with C == KO == G * Cg, Cg in {4, 8, 16, 32, 64}: conv2 of the ResNeXt
// Bottlenecks (aten::convolution(groups=G) and its backward, reached through torchvision from
// virtex/modules/visual_backbones.py:68-74 of the reference).
//
// A grouped convolution is not a small dense one: an output-channel slab depends on its own input-channel slab only, so there is
// no K loop over the channel dimension, every operand byte is used once, and with 4-64 channels per group the arithmetic
// intensity (9 Cg FLOP per byte pair) is far below the gfx950 ridge.  The kernels are therefore STREAMING kernels:
//   * a workgroup (four waves) owns a 64-channel slab = whole groups and walks a run of spatial tiles of TH x 8 output pixels;
//   * per tile the haloed source tile of the slab is staged ONCE in LDS (16-byte loads, zero fill outside the image; a pixel row
//     is 64 channels + 16 bytes of padding, so the 16 pixels of an MFMA fragment fall into different bank groups);
//   * wave t owns the 16 output channels [16 t, 16 t + 16) of the slab.  Its MFMA weight operands never change, so they are built
//     once per workgroup -- the slab's weights (contiguous in [KO][3][3][Cg]) are copied into LDS, and every lane gathers its
//     fragments from there into REGISTERS: block-diagonal for Cg <= 16 (a 16-channel tile spans 16 / Cg groups and reads exactly
//     its own 16 input channels, zeros outside the group), transposed per group with the taps flipped for the input gradient.
//     The LDS bytes of the weights are then reused for the pixel tiles;
//   * K runs over (tap, input channel of the tile) in chunks of 8 bf16 (one lane's share of a 16x16x32 MFMA) or 1 fp32 (16x16x4):
//     Cg <= 16: two taps per K = 32 step, nine taps in five steps (the tenth half-step multiplies zeros); Cg = 32: one step per
//     tap; Cg = 64: two.  The pixel operand of a step is one 16-byte LDS read per lane at (pixel + tap shift, channel chunk);
//   * stride 2 forward reads the staged tile at even positions; the stride-2 input gradient stages the (TH / 2 + 1) x 5 patch of
//     dy a tile of dx depends on and multiplies, per tap, only the pixels whose parity reaches an output pixel (the others get a
//     zero fragment: MFMA issue slots, no bytes);
//   * epilogue straight from the accumulators (a lane holds four consecutive channels of one pixel): + bias, + residual, ReLU.
// The weight gradient contracts over PIXELS: a workgroup owns a slab and a run of tiles, stages the haloed x tile and the dy
// tile, and reads both as k-major MFMA operands with the transposing LDS read (ds_read_b64_tr_b16; fp32: plain reads for 16x16x4).
// The 9 x (KC / 16) accumulator tiles of a wave stay in registers over the whole run; only the block-diagonal part is written,
// as one fp32 partial [KO][9][Cg] per run, and the library's split-K reduction adds the partials into dw in a fixed order: no
// floating-point atomics, identical bits from run to run.
#include "vtx_common.h"

void vtx_splitk_reduce_now(const float* ws, int S, int M, int N, float* C, long ldc, hipStream_t st);

namespace {

constexpr int GC_THREADS = 256;            // four waves: one per 16-channel tile of the 64-channel slab
enum { GC_S1 = 0, GC_FWD_S2 = 1, GC_DGRAD_S2 = 2 };

struct GcGeo {
    int SH, SW;                            // rows / columns of the tensor the taps slide over (x; dy for the input gradient)
    int OH, OW;                            // rows / columns of the tensor a tile is cut from (y; dx; dy for the weight gradient)
    int C, cg_log2;
    int TH;                                // output rows per tile (tiles are TH x 8)
    int th, tw;                            // staged source tile
    float inv_tw;
    int tiles_y, tiles_x, ntiles, tiles_per_wg;
    int transpose;                         // input gradient: per-group transposed weights, taps flipped
    int dy_off, np_pad;                    // weight gradient: LDS byte offset and padded pixel count of the dy tile
};

template <class T> struct GcMma;
template <> struct GcMma<bf16_t> {
    typedef bf16x8_t Frag;
    static constexpr int EPC = 8, KPIX = 32;           // elements of a lane's K chunk; K of one MFMA
    static __device__ __forceinline__ Frag zero() { return Frag{0, 0, 0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ void set(Frag& f, int j, bf16_t v) { f[j] = (short)v; }
    static __device__ __forceinline__ f32x4_t mma(Frag a, Frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct GcMma<float> {
    typedef float Frag;
    static constexpr int EPC = 1, KPIX = 4;
    static __device__ __forceinline__ Frag zero() { return 0.f; }
    static __device__ __forceinline__ void set(Frag& f, int, float v) { f = v; }
    static __device__ __forceinline__ f32x4_t mma(Frag a, Frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <class T> constexpr int gc_pixb() { return 64 * (int)sizeof(T) + 16; }          // LDS bytes of one staged pixel

// four consecutive channels of one pixel <-> fp32 registers
__device__ __forceinline__ void gc_ld4(const float* p, float* v) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
__device__ __forceinline__ void gc_ld4(const bf16_t* p, float* v) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ void gc_st4(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void gc_st4(bf16_t* p, const float* v) { *reinterpret_cast<uint2*>(p) = make_uint2(f2bf2(v[0], v[1]), f2bf2(v[2], v[3])); }

// (tap, chunk within the tap) of K chunk 4 s + q; CPT = chunks per tap.  Two taps share a step only when CPT == 2.
template <int CPT> __device__ __forceinline__ void gc_chunk(int s, int q, int& tap, int& sub) {
    if constexpr (CPT >= 4) { tap = (4 * s) / CPT; sub = (4 * s) % CPT + q; }
    else { tap = 2 * s + (q >> 1); sub = q & 1; }
}

// Stage the 64-channel slab of the th x tw pixel window at (y0, x0) of image n; rows >= rows_valid and pixels outside the image
// are zeros.  Loads of four chunks are requested before any is stored.
template <class T>
__device__ __forceinline__ void gc_stage_tile(char* lds, const T* __restrict__ src, int C, int n, int SH, int SW, int y0, int x0,
                                              int th, int tw, float inv_tw, int rows_valid, int tid) {
    constexpr int CPP = 64 * (int)sizeof(T) / 16, EPV = 16 / (int)sizeof(T), PIXB = gc_pixb<T>();
    const int total = th * tw * CPP;
    for (int i0 = tid; i0 < total; i0 += 4 * GC_THREADS) {
        uint4 v[4]; bool ok[4]; int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + u * GC_THREADS, idc = idx < total ? idx : 0;
            const int pix = idc / CPP, c = idc % CPP;
            const int ty = vtx_fdiv30(pix, tw, inv_tw), tx = pix - ty * tw;
            const int gy = y0 + ty, gx = x0 + tx;
            ok[u] = idx < total && ty < rows_valid && gy >= 0 && gy < SH && gx >= 0 && gx < SW;
            const T* p = ok[u] ? src + ((size_t)(n * SH + gy) * SW + gx) * C + c * EPV : src;
            v[u] = *reinterpret_cast<const uint4*>(p);
            dst[u] = pix * PIXB + c * 16;
        }
        vtx_loads_issued();
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * GC_THREADS < total) *reinterpret_cast<uint4*>(lds + dst[u]) = ok[u] ? v[u] : make_uint4(0u, 0u, 0u, 0u);
    }
}

__device__ __forceinline__ void gc_tile_origin(const GcGeo& g, int tile, int& img, int& oy0, int& ox0) {
    const int per_img = g.tiles_y * g.tiles_x;
    img = tile / per_img;
    const int rem = tile - img * per_img, tyi = rem / g.tiles_x;
    oy0 = tyi * g.TH; ox0 = (rem - tyi * g.tiles_x) * 8;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward / inference forward / input gradient:  out = act(gconv(src, w) + bias + residual)
// ---------------------------------------------------------------------------------------------------------------------
template <class T, int KC, int MODE>
__global__ __launch_bounds__(GC_THREADS) void gconv3x3_kernel(const T* __restrict__ src, const T* __restrict__ w, T* __restrict__ out,
                                                              const float* __restrict__ bias, const T* __restrict__ residual,
                                                              int relu, GcGeo g) {
    typedef GcMma<T> MM;
    typedef typename MM::Frag Frag;
    constexpr int EPC = MM::EPC, CPT = KC / EPC, NSTEP = (9 * CPT + 3) / 4, PIXB = gc_pixb<T>();
    HIP_DYNAMIC_SHARED(char, lds)
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslab = g.C >> 6;
    const int blk = vtx_xcd_major_block(blockIdx.x, gridDim.x);          // neighbouring tiles (shared halos) on one XCD
    const int slab = blk % nslab, tgrp = blk / nslab, c0 = slab * 64;
    const int cgl = g.cg_log2, cg = 1 << cgl;

    // ---- the slab's weights: [64][9][Cg], contiguous -> LDS -> this lane's MFMA fragments (registers, for the whole run)
    {
        const int nchunk = 64 * 9 * cg * (int)sizeof(T) / 16;
        const uint4* wsrc = reinterpret_cast<const uint4*>(w + (size_t)c0 * 9 * cg);
        for (int i = tid; i < nchunk; i += GC_THREADS) reinterpret_cast<uint4*>(lds)[i] = wsrc[i];
    }
    __syncthreads();
    const int cbase = (16 * wave / KC) * KC;                             // first input channel (slab-local) this wave's tile contracts over
    Frag wf[NSTEP];
    {
        const T* wl = reinterpret_cast<const T*>(lds);
        const int own = 16 * wave + n;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            int tap, sub;
            gc_chunk<CPT>(s, q, tap, sub);
            wf[s] = MM::zero();
#pragma unroll
            for (int j = 0; j < EPC; ++j) {
                const int cl = cbase + sub * EPC + j;
                const int ko = g.transpose ? cl : own, ci = g.transpose ? own : cl;
                const bool ok = tap < 9 && (ko >> cgl) == (ci >> cgl);
                const int tt = g.transpose ? 8 - tap : tap;
                const T v = wl[ok ? (ko * 9 + tt) * cg + (ci & (cg - 1)) : 0];
                MM::set(wf[s], j, ok ? v : (T)0);
            }
        }
    }

    const int tile_end = (tgrp + 1) * g.tiles_per_wg < g.ntiles ? (tgrp + 1) * g.tiles_per_wg : g.ntiles;
    const int npix = g.TH * 8, mtiles = (npix + 15) >> 4;
    for (int tile = tgrp * g.tiles_per_wg; tile < tile_end; ++tile) {
        int img, oy0, ox0;
        gc_tile_origin(g, tile, img, oy0, ox0);
        const int sy0 = MODE == GC_S1 ? oy0 - 1 : MODE == GC_FWD_S2 ? 2 * oy0 - 1 : oy0 >> 1;
        const int sx0 = MODE == GC_S1 ? ox0 - 1 : MODE == GC_FWD_S2 ? 2 * ox0 - 1 : ox0 >> 1;
        __syncthreads();                                                 // the weights / the previous tile have been read
        gc_stage_tile<T>(lds, src + c0, g.C, img, g.SH, g.SW, sy0, sx0, g.th, g.tw, g.inv_tw, g.th, tid);
        __syncthreads();
        for (int mt0 = 0; mt0 < mtiles; mt0 += 2) {                      // two independent accumulator chains
            f32x4_t acc[2];
            int ty[2], tx[2], base[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                acc[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                const int p = (mt0 + u) * 16 + n;
                ty[u] = p >> 3; tx[u] = p & 7;
                const int tyc = ty[u] < g.TH ? ty[u] : g.TH - 1;         // the tail of the last fragment: computed, not stored
                constexpr int ST = MODE == GC_FWD_S2 ? 2 : 1;
                base[u] = MODE == GC_DGRAD_S2 ? tyc : (tyc * ST * g.tw + tx[u] * ST) * PIXB;
            }
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                int tap, sub;
                gc_chunk<CPT>(s, q, tap, sub);
                const bool live = tap < 9;
                tap = live ? tap : 8;
                const int r = (tap * 11) >> 5, cc = tap - 3 * r;
                const int coff = (cbase + sub * EPC) * (int)sizeof(T);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    int off; bool ok = live;
                    if constexpr (MODE == GC_DGRAD_S2) {
                        // dx(iy, ix) takes dy((iy + r - 1) / 2, (ix + cc - 1) / 2) through flipped tap (r, cc) when both are even
                        const int a = base[u] + r - 1, b = tx[u] + cc - 1;
                        ok = ok && !((a | b) & 1);
                        off = ok ? ((a >> 1) * g.tw + (b >> 1)) * PIXB + coff : coff;
                    } else {
                        off = base[u] + (r * g.tw + cc) * PIXB + coff;
                    }
                    const Frag f = *reinterpret_cast<const Frag*>(lds + off);
                    acc[u] = MM::mma(wf[s], ok ? f : MM::zero(), acc[u]);
                }
            }
            // lane: channels c0 + 16 wave + 4 q + 0..3 of pixel (ty, tx)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int oy = oy0 + ty[u], ox = ox0 + tx[u];
                if (mt0 + u >= mtiles || ty[u] >= g.TH || oy >= g.OH || ox >= g.OW) continue;
                const int ch = c0 + 16 * wave + 4 * q;
                const size_t o = ((size_t)(img * g.OH + oy) * g.OW + ox) * g.C + ch;
                float v[4] = {acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
                if (bias) {
                    float bv[4];
                    gc_ld4(bias + ch, bv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += bv[i];
                }
                if (residual) {
                    float rv[4];
                    gc_ld4(residual + o, rv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += rv[i];
                }
                if (relu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
                }
                gc_st4(out + o, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient: per-run partials  ws[run][KO][9][Cg]
// ---------------------------------------------------------------------------------------------------------------------
// k-major MFMA operand: element [k = pixel of this lane's K chunk][row = n] of a staged tile.  `off(p)` = LDS byte offset of
// pixel p of the current K step; chb = byte offset of the operand's first channel.
__device__ __forceinline__ vtx_v4s_t gc_read_tr(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) vtx_v4s_t*)p);
}
template <class OFF>
__device__ __forceinline__ bf16x8_t gc_load_k(bf16_t, const char* lds, int n, int q, int chb, OFF off) {
    // the transposing read hands lane n the elements (row n) of the four pixels addressed by lanes 4 j + n / 4: this lane
    // addresses pixel 8 q + n / 4 (+ 4), channels 4 (n % 4) .. + 3
    const int k = 8 * q + (n >> 2), cb = chb + 8 * (n & 3);
    const vtx_v4s_t lo = gc_read_tr(lds + off(k) + cb), hi = gc_read_tr(lds + off(k + 4) + cb);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <class OFF>
__device__ __forceinline__ float gc_load_k(float, const char* lds, int n, int q, int chb, OFF off) {
    return *reinterpret_cast<const float*>(lds + off(q) + chb + 4 * n);
}

template <class T, int KC, int STRIDE>
__global__ __launch_bounds__(GC_THREADS) void gconv3x3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                    float* __restrict__ ws, GcGeo g) {
    typedef GcMma<T> MM;
    typedef typename MM::Frag Frag;
    constexpr int NCT = KC / 16, KPIX = MM::KPIX, PIXB = gc_pixb<T>();
    HIP_DYNAMIC_SHARED(char, lds)
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslab = g.C >> 6;
    const int blk = vtx_xcd_major_block(blockIdx.x, gridDim.x);
    const int slab = blk % nslab, run = blk / nslab, c0 = slab * 64;
    const int cgl = g.cg_log2, cg = 1 << cgl;
    const int cbase = (16 * wave / KC) * KC;

    f32x4_t acc[9][NCT];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[t][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int tile_end = (run + 1) * g.tiles_per_wg < g.ntiles ? (run + 1) * g.tiles_per_wg : g.ntiles;
    const int npix = g.TH * 8, tw = g.tw;
    const char* dyt = lds + g.dy_off;
    for (int tile = run * g.tiles_per_wg; tile < tile_end; ++tile) {
        int img, oy0, ox0;
        gc_tile_origin(g, tile, img, oy0, ox0);
        __syncthreads();
        gc_stage_tile<T>(lds, x + c0, g.C, img, g.SH, g.SW, STRIDE * oy0 - 1, STRIDE * ox0 - 1, g.th, tw, g.inv_tw, g.th, tid);
        gc_stage_tile<T>(lds + g.dy_off, dy + c0, g.C, img, g.OH, g.OW, oy0, ox0, g.np_pad >> 3, 8, 0.125f, g.TH, tid);
        __syncthreads();
        for (int p0 = 0; p0 < g.np_pad; p0 += KPIX) {
            const Frag a = gc_load_k(T(), dyt, n, q, 16 * wave * (int)sizeof(T), [&](int k) { return (p0 + k) * PIXB; });
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int tapoff = ((t / 3) * tw + t % 3) * PIXB;
                // pixels past the tile's end carry dy = 0: their x address is clamped into the staged tile
                auto xoff = [&](int k) {
                    const int p = p0 + k < npix ? p0 + k : npix - 1;
                    return ((p >> 3) * STRIDE * tw + (p & 7) * STRIDE) * PIXB + tapoff;
                };
#pragma unroll
                for (int c = 0; c < NCT; ++c) {
                    const Frag b = gc_load_k(T(), lds, n, q, (cbase + 16 * c) * (int)sizeof(T), xoff);
                    acc[t][c] = MM::mma(a, b, acc[t][c]);
                }
            }
        }
    }
    // lane: dw[ko = 16 wave + 4 q + i][tap][input channel cbase + 16 c + n]; only the block-diagonal part exists
    float* out = ws + (size_t)run * g.C * 9 * cg;
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        const int ci = cbase + 16 * c + n;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ko = 16 * wave + 4 * q + i;
            if ((ko >> cgl) != (ci >> cgl)) continue;
#pragma unroll
            for (int t = 0; t < 9; ++t) out[((size_t)(c0 + ko) * 9 + t) * cg + (ci & (cg - 1))] = acc[t][c][i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int gc_rows_per_tile(int rows, int cap, bool even) {
    int th = vtx_cdiv(rows, vtx_cdiv(rows, cap));
    if (even && (th & 1)) ++th;
    return th;
}

int gc_check(const char* what, int dtype, int N, int H, int W, int C, int G, int stride, int* cg_log2) {
    VTX_CHECK(dtype == VTX_BF16 || dtype == VTX_F32, VTX_ERR_DTYPE, "%s: bad dtype %d", what, dtype);
    VTX_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && G > 0 && C % G == 0, VTX_ERR_SHAPE, "%s: bad shape N=%d H=%d W=%d C=%d groups=%d", what, N, H, W, C, G);
    const int cg = C / G;
    VTX_CHECK(cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64, VTX_ERR_SHAPE,
              "%s: %d channels per group (C=%d, groups=%d); the grouped kernels take 4, 8, 16, 32 or 64", what, cg, C, G);
    VTX_CHECK(C % 64 == 0, VTX_ERR_SHAPE, "%s: C=%d is not a multiple of the 64-channel slab", what, C);
    VTX_CHECK(stride == 1 || stride == 2, VTX_ERR_SHAPE, "%s: stride %d (1 or 2)", what, stride);
    VTX_CHECK((long)N * H * W < VTX_PIXEL_LIMIT, VTX_ERR_SHAPE, "%s: more than 2^30 pixels", what);
    int l = 2;
    while ((1 << l) < cg) ++l;
    *cg_log2 = l;
    return VTX_OK;
}

bool gc_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <class T, int KC, int MODE>
int gc_launch_mode(const GcGeo& g, int grid, size_t lds, const void* src, const void* w, void* out, const float* bias,
                   const void* residual, int relu, double flops, double bytes, hipStream_t st) {
    auto kern = gconv3x3_kernel<T, KC, MODE>;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        vtx_set_error("gconv3x3: %zu bytes of LDS refused", lds);
        return VTX_ERR_LAUNCH;
    }
    VTX_KLAUNCH("gconv3x3", flops, bytes, kern, dim3(grid), dim3(GC_THREADS), lds, st, (const T*)src, (const T*)w, (T*)out, bias,
                (const T*)residual, relu, g);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
template <class T, int KC>
int gc_launch_kc(int mode, const GcGeo& g, int grid, size_t lds, const void* src, const void* w, void* out, const float* bias,
                 const void* residual, int relu, double flops, double bytes, hipStream_t st) {
    if (mode == GC_S1) return gc_launch_mode<T, KC, GC_S1>(g, grid, lds, src, w, out, bias, residual, relu, flops, bytes, st);
    if (mode == GC_FWD_S2) return gc_launch_mode<T, KC, GC_FWD_S2>(g, grid, lds, src, w, out, bias, residual, relu, flops, bytes, st);
    return gc_launch_mode<T, KC, GC_DGRAD_S2>(g, grid, lds, src, w, out, bias, residual, relu, flops, bytes, st);
}

// src [N][SH][SW][C] -> out [N][OH][OW][C]; dgrad: src = dy, out = dx
int gc_run(const char* what, int dtype, int N, int H, int W, int C, int G, int stride, bool dgrad, const void* src, const void* w,
           void* out, const float* bias, const void* residual, int relu, hipStream_t st) {
    int cgl;
    if (int e = gc_check(what, dtype, N, H, W, C, G, stride, &cgl)) return e;
    VTX_CHECK(src && w && out, VTX_ERR_ARG, "%s: null pointer", what);
    VTX_CHECK(gc_aligned(src) && gc_aligned(w) && gc_aligned(out) && gc_aligned(bias) && gc_aligned(residual), VTX_ERR_ARG,
              "%s: pointers must be 16-byte aligned", what);
    const int H2 = (H - 1) / stride + 1, W2 = (W - 1) / stride + 1;           // the convolution's output extent
    const int mode = stride == 1 ? GC_S1 : dgrad ? GC_DGRAD_S2 : GC_FWD_S2;
    GcGeo g{};
    g.SH = dgrad ? H2 : H; g.SW = dgrad ? W2 : W;
    g.OH = dgrad ? H : H2; g.OW = dgrad ? W : W2;
    g.C = C; g.cg_log2 = cgl; g.transpose = dgrad ? 1 : 0;
    g.TH = gc_rows_per_tile(g.OH, mode == GC_FWD_S2 ? 8 : 16, mode == GC_DGRAD_S2);
    g.th = mode == GC_S1 ? g.TH + 2 : mode == GC_FWD_S2 ? 2 * g.TH + 1 : g.TH / 2 + 1;
    g.tw = mode == GC_S1 ? 10 : mode == GC_FWD_S2 ? 17 : 5;
    g.inv_tw = 1.0f / (float)g.tw;
    g.tiles_y = vtx_cdiv(g.OH, g.TH); g.tiles_x = vtx_cdiv(g.OW, 8);
    g.ntiles = N * g.tiles_y * g.tiles_x;
    const int nslab = C / 64, cg = C / G;
    // a workgroup keeps its weight fragments over a run of tiles; about eight workgroups per CU keep the staging of one under
    // the MFMAs of the others
    g.tiles_per_wg = vtx_cdiv((long)g.ntiles * nslab, 2048);
    const int grid = vtx_cdiv(g.ntiles, g.tiles_per_wg) * nslab;
    const size_t esz = dtype == VTX_BF16 ? 2 : 4;
    const size_t pixb = 64 * esz + 16;
    const size_t lds_w = (size_t)64 * 9 * cg * esz, lds_t = (size_t)g.th * g.tw * pixb;
    const size_t lds = lds_w > lds_t ? lds_w : lds_t;
    const double opix = (double)N * g.OH * g.OW, spix = (double)N * g.SH * g.SW;
    const double flops = 2.0 * opix * C * 9 * cg;
    const double bytes = esz * ((opix + spix) * C + 9.0 * C * cg + (residual ? opix * C : 0));
#define GC_GO(T_, KC_) return gc_launch_kc<T_, KC_>(mode, g, grid, lds, src, w, out, bias, residual, relu, flops, bytes, st)
    if (dtype == VTX_BF16) { if (cg <= 16) GC_GO(bf16_t, 16); if (cg == 32) GC_GO(bf16_t, 32); GC_GO(bf16_t, 64); }
    if (cg <= 16) GC_GO(float, 16);
    if (cg == 32) GC_GO(float, 32);
    GC_GO(float, 64);
#undef GC_GO
}

template <class T, int KC, int STRIDE>
int gc_wgrad_launch(const GcGeo& g, int grid, size_t lds, const void* x, const void* dy, float* ws, double flops, double bytes,
                    hipStream_t st) {
    auto kern = gconv3x3_wgrad_kernel<T, KC, STRIDE>;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        vtx_set_error("gconv3x3_wgrad: %zu bytes of LDS refused", lds);
        return VTX_ERR_LAUNCH;
    }
    VTX_KLAUNCH("gconv3x3_wgrad", flops, bytes, kern, dim3(grid), dim3(GC_THREADS), lds, st, (const T*)x, (const T*)dy, ws, g);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

}  // namespace

/* aten::convolution(groups=G) of conv2 of torchvision's ResNeXt Bottleneck, virtex/modules/visual_backbones.py:68-74 of the reference */
extern "C" int vtx_gconv3x3_fwd(int dtype, int N, int H, int W, int C, int G, int stride, const void* x, const void* w, void* y,
                                void* stream) {
    return gc_run("gconv3x3_fwd", dtype, N, H, W, C, G, stride, false, x, w, y, nullptr, nullptr, 0, (hipStream_t)stream);
}

extern "C" int vtx_gconv3x3_infer(int dtype, int N, int H, int W, int C, int G, int stride, const void* x, const void* w,
                                  const float* bias, const void* residual, int relu, void* y, void* stream) {
    return gc_run("gconv3x3_infer", dtype, N, H, W, C, G, stride, false, x, w, y, bias, residual, relu, (hipStream_t)stream);
}

extern "C" int vtx_gconv3x3_dgrad(int dtype, int N, int H, int W, int C, int G, int stride, const void* dy, const void* w, void* dx,
                                  const void* residual, void* stream) {
    return gc_run("gconv3x3_dgrad", dtype, N, H, W, C, G, stride, true, dy, w, dx, nullptr, residual, 0, (hipStream_t)stream);
}

extern "C" int vtx_gconv3x3_wgrad(int dtype, int N, int H, int W, int C, int G, int stride, const void* x, const void* dy, float* dw,
                                  float* workspace, long workspace_floats, void* stream) {
    int cgl;
    if (int e = gc_check("gconv3x3_wgrad", dtype, N, H, W, C, G, stride, &cgl)) return e;
    VTX_CHECK(x && dy && dw && workspace, VTX_ERR_ARG, "gconv3x3_wgrad: null pointer");
    VTX_CHECK(gc_aligned(x) && gc_aligned(dy) && gc_aligned(dw) && gc_aligned(workspace), VTX_ERR_ARG,
              "gconv3x3_wgrad: pointers must be 16-byte aligned");
    const int cg = C / G, nslab = C / 64;
    const long slice = (long)C * 9 * cg;
    VTX_CHECK(workspace_floats >= slice, VTX_ERR_ARG, "gconv3x3_wgrad: the workspace holds %ld floats, one partial needs %ld",
              workspace_floats, slice);
    GcGeo g{};
    g.SH = H; g.SW = W;
    g.OH = (H - 1) / stride + 1; g.OW = (W - 1) / stride + 1;
    g.C = C; g.cg_log2 = cgl;
    g.TH = gc_rows_per_tile(g.OH, stride == 1 ? 16 : 8, false);
    g.th = stride == 1 ? g.TH + 2 : 2 * g.TH + 1;
    g.tw = stride == 1 ? 10 : 17;
    g.inv_tw = 1.0f / (float)g.tw;
    g.tiles_y = vtx_cdiv(g.OH, g.TH); g.tiles_x = vtx_cdiv(g.OW, 8);
    g.ntiles = N * g.tiles_y * g.tiles_x;
    const size_t esz = dtype == VTX_BF16 ? 2 : 4, pixb = 64 * esz + 16;
    g.np_pad = ((g.TH * 8 + 31) / 32) * 32;
    g.dy_off = (int)((size_t)g.th * g.tw * pixb);
    const size_t lds = (size_t)g.dy_off + (size_t)g.np_pad * pixb;
    // runs of tiles: about four workgroups per CU, at most what the workspace holds
    long nruns = 1024 / nslab > 0 ? 1024 / nslab : 1;
    if (nruns > g.ntiles) nruns = g.ntiles;
    if (nruns > workspace_floats / slice) nruns = workspace_floats / slice;
    g.tiles_per_wg = vtx_cdiv(g.ntiles, nruns);
    nruns = vtx_cdiv(g.ntiles, g.tiles_per_wg);
    const int grid = (int)nruns * nslab;
    const double opix = (double)N * g.OH * g.OW;
    const double flops = 2.0 * opix * C * 9 * cg;
    const double bytes = esz * ((opix + (double)N * H * W) * C) + 4.0 * nruns * slice;
    hipStream_t st = (hipStream_t)stream;
    int e;
#define GC_WG(T_, KC_) e = stride == 1 ? gc_wgrad_launch<T_, KC_, 1>(g, grid, lds, x, dy, workspace, flops, bytes, st) \
                                       : gc_wgrad_launch<T_, KC_, 2>(g, grid, lds, x, dy, workspace, flops, bytes, st)
    if (dtype == VTX_BF16) { if (cg <= 16) GC_WG(bf16_t, 16); else if (cg == 32) GC_WG(bf16_t, 32); else GC_WG(bf16_t, 64); }
    else { if (cg <= 16) GC_WG(float, 16); else if (cg == 32) GC_WG(float, 32); else GC_WG(float, 64); }
#undef GC_WG
    if (e) return e;
    vtx_splitk_reduce_now(workspace, (int)nruns, C, 9 * cg, dw, 9L * cg, st);       // dw += the partials, in run order
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
