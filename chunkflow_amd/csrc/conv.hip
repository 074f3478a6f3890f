// Hand-written MFMA 3x3x3 convolution for gfx950 — the RSUNet ResBlock
// conv (C == K in {28, 36, 48, 64}, stride 1, pad 1, NDHWC f32).
//
// WHAT SHIPS (every kernel here is reached through the C ABI by its
// arguments alone — no environment variable selects a kernel — and is
// pinned bit-exactly by tests/test_conv_exact.py):
//   cfx_conv3_ndhwc        k_conv3 slab, C = 28/36/48/64
//   cfx_conv3_ndhwc_w32    k_conv3_w32 (32x32x2), C = 28
//   cfx_conv3_ndhwc_zring  k_conv3_zring_pl, C = 28 [111 TF] (one launch,
//                          two 16-wide tiles, LDS 157.2 KB) and 36 [117
//                          TF] (two launches: columns 0..15 + the 4x4x1
//                          block tile 32..35, 155.5 KB, then 16..31,
//                          140.0 KB); block columns are summed per
//                          k-slice, then (s0+s2)+(s1+s3) across lanes;
//                          k_conv3_zring_dw, C = 48 (37 TF, slower than
//                          the slab; kept as the only C=48 ring route)
//   cfx_conv3_ndhwc_bf16   k_conv3_zring_bf16_a, C = 28 [610-646 TF];
//                          k_conv3_zring_bf16_s sliced c-half x j-tile
//                          schedule, C = 36 [249 TF] and 48
// The optimisation ladder these came out of (the plain ring, the 4-slot
// and swizzled rings, 16x16x32, deferred epilogue, the phase ablations)
// is recorded with its numbers in DESIGN.md §10/§10-r2/§11; its source
// is in git history.
//
// MIOpen's ck-xdlops kernels reach ~58 TF/s f32 on these shapes; the small
// channel depth (N-dim 28..64) starves generic implicit GEMM. This kernel
// exploits the structure directly:
//   * conv = sum over the 27 taps of GEMM( input-shifted [M x C],
//     W_tap [C x K] ) — computed per workgroup from ONE LDS-resident input
//     slab (output tile + 3x3x3 halo), so each input value is read from
//     HBM once per tile (x-halo 2/34, y-halo 2/TY+2, z-halo shared);
//   * v_mfma_f32_16x16x4_f32 (exact f32, 155 TF ceiling): D tile = 16
//     x-positions x 16 output channels, reduction 4 input channels per
//     instruction; A operand = one LDS dword per lane (bank-conflict-free
//     by construction: the lane address stride C mod 32 is kept out of
//     {0, 16} by padding the slab's x-stride), B operand = one weight
//     dword per lane, staged through LDS per tap and reused by every
//     M-tile of the wave;
//   * fused bias + optional ELU + optional residual add in the epilogue.
//
// Geometry per workgroup (template TY): output tile TZ=2 x TY x TX=32
// voxels, 4 waves; TY=4 for C<=36 (slab <= 118 KB), TY=2 for C in
// {48, 64} (slab <= 148 KB incl. padding). Weights are (27, C, K) f32
// (prepared host-side from torch's (K, C, 3, 3, 3)).
#include <hip/hip_runtime.h>

#include "cfx_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int padc(int C) {  // slab voxel stride: keep (stride mod 32)
    return (C % 32 == 0 || C % 32 == 16) ? C + 4 : C;  // out of {0, 16}
}

// Generic wave->tile mapping: the workgroup's TZ x TY x (TX/16) 16-wide
// m-tiles are dealt round-robin to NW = NTHREADS/64 waves; NTHREADS=512
// puts 2 waves on each SIMD (the co-resident wave hides LDS latency the
// single wave of the 256-thread shape cannot). TAPG = taps whose weights
// are staged per barrier pair.
template <int C, int K, int TZv, int TY, int TX, int TAPG, int NTHREADS>
__global__ __launch_bounds__(NTHREADS, 1) void k_conv3(
    const float* __restrict__ in,    // (N, D, H, W, C) channels-last
    const float* __restrict__ wgt,   // (27, C, K)
    const float* __restrict__ bias,  // (K)
    const float* __restrict__ res,   // optional residual, same layout as out
    float* __restrict__ out,         // (N, D, H, W, K)
    int N, int D, int H, int W, int do_elu) {
    constexpr int PC = padc(C);
    constexpr int SX = TX + 2;            // slab x extent (halo)
    constexpr int SY = TY + 2;
    constexpr int SZ = TZv + 2;
    constexpr int KK = C / 4;             // reduction steps per tap
    constexpr int NT = (K + 15) / 16;     // 16-wide output-channel tiles
    constexpr int NW = NTHREADS / 64;     // waves per workgroup
    constexpr int XT = TX / 16;           // 16-wide x tiles
    constexpr int M_TILES = (TZv * TY * XT) / NW;  // m-tiles per wave
    static_assert((TZv * TY * XT) % NW == 0, "tiles must split evenly");

    __shared__ float slab[SZ * SY * SX * PC];
    // TAPG taps x NT 16-wide K tiles, each a [C][16] block (the 16-dword
    // row stride keeps the B-fragment reads bank-conflict-free)
    __shared__ float wtile[TAPG * NT * C * 16];

    const int bx = blockIdx.x;                  // x block
    const int by = blockIdx.y;                  // y block
    const int bzn = blockIdx.z;                 // fused (n, z-block)
    const int zblocks = (D + TZv - 1) / TZv;
    const int n = bzn / zblocks;
    const int z0 = (bzn % zblocks) * TZv;
    const int y0 = by * TY;
    const int x0 = bx * TX;

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;

    // ---- stage the input slab (zero-padded at volume borders) ----------
    // float4 runs along C (C % 4 == 0 for all widths). Loads are issued
    // UNCONDITIONALLY from clamped addresses and zeroed afterwards — a
    // per-element guarded load makes hipcc branch around each load and
    // drain vmcnt per element (cdna_hip_programming.md §5 trap (c)), which
    // was the dominant cost of the first version at 1 workgroup/CU.
    {
        const int c4n = C / 4;
        const int vox = SZ * SY * SX;
        const bool interior = z0 >= 1 && z0 + TZv + 1 <= D && y0 >= 1 &&
                              y0 + TY + 1 <= H && x0 >= 1 &&
                              x0 + TX + 1 <= W;
        const float* base =
            in + ((((long long)n * D + z0 - 1) * H + y0 - 1) * W + x0 - 1)
                 * C;
        if (interior) {
            for (int idx = tid; idx < vox * c4n; idx += NTHREADS) {
                const int c4 = idx % c4n;
                const int v = idx / c4n;
                const int sx = v % SX;
                const int sy = (v / SX) % SY;
                const int sz = v / (SX * SY);
                const f32x4 val = *reinterpret_cast<const f32x4*>(
                    base + (((long long)sz * H + sy) * W + sx) * C +
                    c4 * 4);
                *reinterpret_cast<f32x4*>(
                    &slab[((sz * SY + sy) * SX + sx) * PC + c4 * 4]) = val;
            }
        } else {
            for (int idx = tid; idx < vox * c4n; idx += NTHREADS) {
                const int c4 = idx % c4n;
                const int v = idx / c4n;
                const int sx = v % SX;
                const int sy = (v / SX) % SY;
                const int sz = v / (SX * SY);
                const int gz = z0 + sz - 1;
                const int gy = y0 + sy - 1;
                const int gx = x0 + sx - 1;
                const bool ok = gz >= 0 && gz < D && gy >= 0 && gy < H &&
                                gx >= 0 && gx < W;
                const int cz = ok ? gz : 0;
                const int cy = ok ? gy : 0;
                const int cx = ok ? gx : 0;
                f32x4 val = *reinterpret_cast<const f32x4*>(
                    in + ((((long long)n * D + cz) * H + cy) * W + cx) * C +
                    c4 * 4);
                if (!ok) val = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(
                    &slab[((sz * SY + sy) * SX + sx) * PC + c4 * 4]) = val;
            }
        }
    }
    __syncthreads();

    // ---- wave tile origins (generic round-robin deal) -------------------
    int tmz[M_TILES], tmy[M_TILES], tmx[M_TILES];
#pragma unroll
    for (int m = 0; m < M_TILES; ++m) {
        const int g = wave * M_TILES + m;
        tmx[m] = (g % XT) * 16;
        tmy[m] = (g / XT) % TY;
        tmz[m] = g / (XT * TY);
    }

    f32x4 acc[M_TILES][NT];
#pragma unroll
    for (int m = 0; m < M_TILES; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
            acc[m][t] = {0.f, 0.f, 0.f, 0.f};

    const int a_row = lane & 15;   // x within the m-tile (A row, B col)
    const int a_k = lane >> 4;     // reduction sub-index (0..3)
    const int col16 = lane & 15;

    // ---- 27 taps in groups of TAPG -------------------------------------
    static_assert(27 % TAPG == 0, "TAPG must divide 27");
    for (int g = 0; g < 27 / TAPG; ++g) {
        // stage the group's weights: TAPG x NT blocks of [C][16]
        for (int idx = tid; idx < TAPG * NT * C * 16;
             idx += NTHREADS) {
            const int j = idx & 15;
            const int c = (idx >> 4) % C;
            const int nt = (idx >> 4) / C % NT;
            const int tl = (idx >> 4) / C / NT;
            const int jg = nt * 16 + j;
            wtile[idx] = jg < K
                ? wgt[((long long)(g * TAPG + tl) * C + c) * K + jg]
                : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tl = 0; tl < TAPG; ++tl) {
            const int tap = g * TAPG + tl;
            const int dz = tap / 9 - 1;
            const int dy = (tap / 3) % 3 - 1;
            const int dx = tap % 3 - 1;
            // kk outer / m inner: the accumulator chains interleave,
            // hiding the 40-cycle dependent-MFMA latency (the 16x16x4
            // issue interval is 32) at one wave per SIMD
            const float* arow[M_TILES];
#pragma unroll
            for (int m = 0; m < M_TILES; ++m) {
                arow[m] = &slab[(((1 + tmz[m] + dz) * SY +
                                  (1 + tmy[m] + dy)) * SX +
                                 (1 + tmx[m] + dx)) * PC + a_row * PC + a_k];
            }
            const float* wblk = &wtile[tl * NT * C * 16];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    // A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]
                    const float b =
                        wblk[(nt * C + kk * 4 + a_k) * 16 + col16];
#pragma unroll
                    for (int m = 0; m < M_TILES; ++m) {
                        const float a = arow[m][kk * 4];
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            a, b, acc[m][nt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- epilogue: D[row = (lane>>4)*4 + reg][col = lane&15] -------------
    const int col = lane & 15;
    const int rbase = (lane >> 4) * 4;
#pragma unroll
    for (int m = 0; m < M_TILES; ++m) {
        const int gz = z0 + tmz[m];
        const int gy = y0 + tmy[m];
        if (gz >= D || gy >= H) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = t * 16 + col;
            if (j >= K) continue;
            const float bj = bias ? bias[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gx = x0 + tmx[m] + rbase + r;
                if (gx >= W) continue;
                long long o =
                    ((((long long)n * D + gz) * H + gy) * W + gx) * K + j;
                float v = acc[m][t][r] + bj;
                if (res) v += res[o];
                if (do_elu) v = v > 0.f ? v : expm1f(v);
                out[o] = v;
            }
        }
    }
}

}  // namespace

extern "C" int cfx_conv3_ndhwc(cfx_ctx* ctx, const float* in,
                               const float* wgt, const float* bias,
                               const float* residual, float* out, int N,
                               int D, int H, int W, int C, int K,
                               int do_elu) {
    if (C != K) {
        g_err = "cfx_conv3_ndhwc: only C == K widths are instantiated";
        return -1;
    }
    // LDS budget per width (slab + wtile <= 160 KiB); NTHREADS=512 puts
    // 2 waves per SIMD where the slab allows it
#define CFX_CONV_CASE(CW, TZV, TYV, TXV, TAPGV, NTH)                         \
    case CW: {                                                               \
        const int zb = (D + TZV - 1) / TZV;                                  \
        dim3 grid((W + TXV - 1) / TXV, (H + TYV - 1) / TYV,                  \
                  (unsigned)(N * zb));                                       \
        hipLaunchKernelGGL((k_conv3<CW, CW, TZV, TYV, TXV, TAPGV, NTH>),     \
                           grid, dim3(NTH), 0, ctx->stream, in, wgt, bias,   \
                           residual, out, N, D, H, W, do_elu);               \
        return 0;                                                            \
    }
    double flops = 2.0 * 27.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV, flops, [&] {
        switch (C) {
            // 28: slab 3*10*34*28*4 = 114 KB + wtile 10.5 KB (TZ1 TY8,
            // 8 waves)
            CFX_CONV_CASE(28, 1, 8, 32, 3, 512)
            // 36: slab 3*10*34*36*4 = 147 KB + wtile 4.5 KB (TAPG 1)
            CFX_CONV_CASE(36, 1, 8, 32, 1, 512)
            // 48: slab 3*6*34*52*4 = 127 KB + wtile 9.2 KB (TZ1 TY4,
            // 8 waves -> 1 m-tile per wave)
            CFX_CONV_CASE(48, 1, 4, 32, 1, 512)
            // 64: slab 3*6*18*68*4 = 86 KB + wtile 16.4 KB (TZ1 TY4 TX16;
            // 8 waves x ... 1*4*1 = 4 tiles < 8 waves -> use 256 threads)
            CFX_CONV_CASE(64, 2, 2, 16, 1, 256)
            default:
                g_err = "cfx_conv3_ndhwc: unsupported channel width";
                return -1;
        }
    });
#undef CFX_CONV_CASE
}

namespace {

// 32x32x2 variant (C == K <= 32): one 32-x-position x 32-channel D tile
// per wave, single accumulator chain (the 32x32x2 dependent latency equals
// its 64-cycle issue interval, so one chain sustains the full rate), and
// one A + one B LDS dword per 4096 flops (3x fewer LDS reads per flop than
// the 16x16x4 path). Slab layout [z][y][c][x] (x fastest) makes the
// A-fragment read (lanes 0..31 = consecutive x) trivially conflict-free.
template <int C, int K, int TY, int TAPG>
__global__ __launch_bounds__(512, 1) void k_conv3_w32(
    const float* __restrict__ in, const float* __restrict__ wgt,
    const float* __restrict__ bias, const float* __restrict__ res,
    float* __restrict__ out, int N, int D, int H, int W, int do_elu) {
    constexpr int TX = 32;
    constexpr int SX = TX + 2;
    constexpr int SY = TY + 2;
    constexpr int SZ = 3;                // TZ = 1
    constexpr int KK = C / 2;            // reduction pairs per tap
    static_assert(K <= 32 && C % 2 == 0, "");

    __shared__ float slab[SZ * SY * C * SX];
    __shared__ float wtile[TAPG * C * 32];

    const int zblocks = D;               // TZ = 1
    const int n = blockIdx.z / zblocks;
    const int z0 = blockIdx.z % zblocks;
    const int y0 = blockIdx.y * TY;
    const int x0 = blockIdx.x * TX;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;           // 0..7 -> y row
    const int lane = tid & 63;

    // ---- stage the slab: read NDHWC float4 runs, scatter to [c][x] ------
    {
        const int c4n = C / 4;
        const bool interior = z0 >= 1 && z0 + 2 <= D && y0 >= 1 &&
                              y0 + TY + 1 <= H && x0 >= 1 &&
                              x0 + TX + 1 <= W;
        for (int idx = tid; idx < SZ * SY * SX * c4n; idx += 512) {
            const int c4 = idx % c4n;
            const int v = idx / c4n;
            const int sx = v % SX;
            const int sy = (v / SX) % SY;
            const int sz = v / (SX * SY);
            const int gz = z0 + sz - 1;
            const int gy = y0 + sy - 1;
            const int gx = x0 + sx - 1;
            f32x4 val;
            if (interior) {
                val = *reinterpret_cast<const f32x4*>(
                    in + ((((long long)n * D + gz) * H + gy) * W + gx) * C +
                    c4 * 4);
            } else {
                const bool ok = gz >= 0 && gz < D && gy >= 0 && gy < H &&
                                gx >= 0 && gx < W;
                val = *reinterpret_cast<const f32x4*>(
                    in + ((((long long)n * D + (ok ? gz : 0)) * H +
                           (ok ? gy : 0)) * W + (ok ? gx : 0)) * C +
                    c4 * 4);
                if (!ok) val = {0.f, 0.f, 0.f, 0.f};
            }
            float* base = &slab[((sz * SY + sy) * C + c4 * 4) * SX + sx];
            base[0 * SX] = val.x;
            base[1 * SX] = val.y;
            base[2 * SX] = val.z;
            base[3 * SX] = val.w;
        }
    }
    __syncthreads();

    typedef float f32x16 __attribute__((ext_vector_type(16)));
    f32x16 acc = {};
    const int ax = lane & 31;            // A row (x), B col (j)
    const int ak = lane >> 5;            // reduction sub-index (0..1)

    static_assert(27 % TAPG == 0, "");
    for (int g = 0; g < 27 / TAPG; ++g) {
        for (int idx = tid; idx < TAPG * C * 32; idx += 512) {
            const int j = idx & 31;
            const int c = (idx >> 5) % C;
            const int tl = (idx >> 5) / C;
            wtile[idx] = j < K
                ? wgt[((long long)(g * TAPG + tl) * C + c) * K + j]
                : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tl = 0; tl < TAPG; ++tl) {
            const int tap = g * TAPG + tl;
            const int dz = tap / 9 - 1;
            const int dy = (tap / 3) % 3 - 1;
            const int dx = tap % 3 - 1;
            const float* arow =
                &slab[((1 + dz) * SY + (1 + wave + dy)) * C * SX +
                      (1 + dx) + ax];
            const float* wrow = &wtile[tl * C * 32 + ax];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const float a = arow[(kk * 2 + ak) * SX];
                const float b = wrow[(kk * 2 + ak) * 32];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0,
                                                           0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: D[row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)][col] -----
    const int gz = z0;
    const int gy = y0 + wave;
    const int j = lane & 31;
    if (gy < H && j < K) {
        const float bj = bias ? bias[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int gx = x0 + row;
            if (gx >= W) continue;
            long long o =
                ((((long long)n * D + gz) * H + gy) * W + gx) * K + j;
            float v = acc[r] + bj;
            if (res) v += res[o];
            if (do_elu) v = v > 0.f ? v : expm1f(v);
            out[o] = v;
        }
    }
}

}  // namespace

// 32x32x2 path for C == K <= 32 (currently instantiated for 28); falls
// back to the 16x16x4 path when CFX_CONV_W32=0
extern "C" int cfx_conv3_ndhwc_w32(cfx_ctx* ctx, const float* in,
                                   const float* wgt, const float* bias,
                                   const float* residual, float* out, int N,
                                   int D, int H, int W, int C, int K,
                                   int do_elu) {
    if (C != 28 || K != 28) {
        g_err = "cfx_conv3_ndhwc_w32: only C == K == 28 instantiated";
        return -1;
    }
    dim3 grid((W + 31) / 32, (H + 7) / 8, (unsigned)(N * D));
    double flops = 2.0 * 27.0 * 28 * 28 * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV, flops, [&] {
        hipLaunchKernelGGL((k_conv3_w32<28, 28, 8, 3>), grid, dim3(512), 0,
                           ctx->stream, in, wgt, bias, residual, out, N, D,
                           H, W, do_elu);
        return 0;
    });
}

namespace {

// Persistent-z ring: the workgroup walks ALL z planes of its (y, x)
// tile. Weights for all 27 taps stay LDS-RESIDENT for the whole workgroup
// (staged once, amortized over D planes — per-tap-group re-staging was
// most of the per-z overhead), and the input slab is a 3-plane ring with
// ONE ~20 KB plane staged per z. LDS: ring 3 x SY x SX x C (60.5 KB at
// C=28, TY=8, TX=16) + weights 27 x C x (16 NT + 4 NT4) (96.8 KB) =
// 157 KB (per width: below).
// Software-pipelined: the NEXT plane's global loads are issued into
// registers first, the 18 taps that only touch the two already-resident
// planes run while those loads are in flight, then the registers drain to
// the ring slot and ONE barrier per z releases the last 9 taps: iteration
// z's store targets the slot plane z-2 occupied, whose last readers (dzi=0
// of iteration z-1) sit before iteration z-1's barrier. Per z the order of
// memory traffic is: plane loads | 18 taps | plane stores, barrier |
// residual loads | 9 taps | outputs finished in registers | stores back to
// back — no wait ever sees a pending store (DESIGN.md §10-r2 item 8 has
// what the assembly looked like before and what each part was worth).
//
// A ragged output width (K = 36 against the 16-wide tile) rides on
// NT4 BLOCK TILES of 4 columns, starting at column J4, computed by
// v_mfma_f32_4x4x1_16b_f32 out of the same A fragment: the lane's
// in[pos = lane & 15][c = 4 kk + (lane >> 4)] read as 16 blocks of 4 lanes
// is block b = lane >> 2 = (position group b & 3, k-slice b >> 2), row
// lane & 3; with B = w[c = 4 kk + (lane >> 4)][J4 + 4 t + (lane & 3)] one
// instruction is a 16-position x 4-column x 4-channel product at a quarter
// of a 16x16x4 and no zero column (layout and issue cost:
// tools/mfma_layout_probe.py --f32-blocks, profiles/zring_blocks_probe
// .json). Register i of lane l then holds the k-slice l >> 4 partial of
// position 4 ((l >> 2) & 3) + i, column l & 3; once per z the four
// k-slices are added as (s_q + s_q^2) + (s_q^1 + s_q^3) — the same value
// in every lane, xor-32 then xor-16 — and lane l keeps row l >> 4, so four
// consecutive lanes store the 16 contiguous bytes of one position. The
// block wall [tap][t][c][4] sits behind the 16-wide wall; a wave's read
// of it touches 16 consecutive floats.
//   C=28: one launch, NT=2, NT4=0: wall 96.8 KB, ring 60.5 KB = 157.2 KB
//         (NT=1 + NT4=3 at J4=16 fits in 145.2 KB and was slower: three
//         block MFMAs cost 28-30 issue cycles against the 32 of the
//         padded tile they replace, and bring three more LDS reads)
//   C=36: launch A j0=0, NT=1 + NT4=1 at J4=32: wall 62.2 + 15.6 KB, ring
//         77.8 KB = 155.5 KB; launch B j0=16, NT=1, NT4=0: 140.0 KB
template <int C, int K, int TY, int TX, int NTK, int NT4, int J4>
__global__ __launch_bounds__(512, 1) void k_conv3_zring_pl(
    const float* __restrict__ in, const float* __restrict__ wgt,
    const float* __restrict__ bias, const float* __restrict__ res,
    float* __restrict__ out, int N, int D, int H, int W, int do_elu,
    int j0, int wvec) {
    constexpr int PC = padc(C);
    constexpr int SX = TX + 2;
    constexpr int SY = TY + 2;
    constexpr int KK = C / 4;
    constexpr int NT = NTK;
    constexpr int N4 = NT4 > 0 ? NT4 : 1;  // array extent (unused at NT4=0)
    constexpr int NW = 8;
    constexpr int XT = TX / 16;
    constexpr int M_TILES = (TY * XT) / NW;
    constexpr int C4N = C / 4;
    constexpr int LV = (SY * SX * C4N + 511) / 512;  // loads held per thread
    constexpr int W16 = 27 * NT * C * 16;            // 16-wide wall, floats
    constexpr int W16V4 = W16 / 4;
    constexpr int WV4 = W16V4 + 27 * NT4 * C;        // wall size in float4
    constexpr int WL = (WV4 + 511) / 512;            // wall float4 per thread
    constexpr bool SPLIT = NT == 1;  // 16-wide chain split by kk parity
    static_assert((TY * XT) % NW == 0, "");
    static_assert(NT4 == 0 || (J4 % 4 == 0 && J4 + 4 * NT4 <= K), "");

    __shared__ __attribute__((aligned(16))) float ring[3 * SY * SX * PC];
    __shared__ __attribute__((aligned(16))) float wall[WV4 * 4];

    const int n = blockIdx.z;
    const int y0 = blockIdx.y * TY;
    const int x0 = blockIdx.x * TX;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;

    // Weight wall, staged once per workgroup. wvec (host-checked: wgt
    // 16-byte aligned, K % 4 == 0, and j0 % 4 == 0 by construction): a
    // float4 of a (tap, c) weight row is four consecutive j of one wall
    // row and lies either wholly below K or wholly in the zero padding,
    // so the wall goes through registers as ONE batch of float4 loads
    // from clamped addresses with the zero-select deferred to the LDS
    // store, like plane_load/plane_store. The scalar loop is the
    // fallback for a misaligned weight tensor: one dword per dependent
    // L2 round trip.
    auto wall_load = [&](f32x4 (&wv)[WL], bool (&wk)[WL]) {
#pragma unroll
        for (int li = 0; li < WL; ++li) {
            const int idx = min(tid + li * 512, WV4 - 1);
            // a float4 past the 16-wide wall is one whole (tap, t, c) row
            // of a block tile, always below K
            const bool blk = NT4 > 0 && idx >= W16V4;
            const int row = blk ? idx - W16V4 : idx >> 2;
            const int c = row % C;
            const int nt = blk ? row / C % N4 : row / C % NT;
            const int tap = blk ? row / C / N4 : row / C / NT;
            const int jg = blk ? J4 + nt * 4 : j0 + nt * 16 + (idx & 3) * 4;
            wk[li] = jg < K;
            wv[li] = *reinterpret_cast<const f32x4*>(
                wgt + ((long long)tap * C + c) * K + (jg < K ? jg : 0));
        }
    };
    auto wall_store = [&](const f32x4 (&wv)[WL], const bool (&wk)[WL]) {
#pragma unroll
        for (int li = 0; li < WL; ++li) {
            const int idx = tid + li * 512;
            if (idx >= WV4) break;
            *reinterpret_cast<f32x4*>(&wall[idx * 4]) =
                wk[li] ? wv[li] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if (!wvec) {
        for (int idx = tid; idx < W16; idx += 512) {
            const int j = idx & 15;
            const int c = (idx >> 4) % C;
            const int nt = (idx >> 4) / C % NT;
            const int tap = (idx >> 4) / C / NT;
            const int jg = j0 + nt * 16 + j;
            wall[idx] =
                jg < K ? wgt[((long long)tap * C + c) * K + jg] : 0.f;
        }
        for (int idx = tid; idx < 27 * NT4 * C * 4; idx += 512) {
            const int c = (idx >> 2) % C;
            const int t = (idx >> 2) / C % N4;
            const int tap = (idx >> 2) / C / N4;
            wall[W16 + idx] = wgt[((long long)tap * C + c) * K + J4 +
                                  t * 4 + (idx & 3)];
        }
    }

    const bool xy_interior = y0 >= 1 && y0 + TY + 1 <= H && x0 >= 1 &&
                             x0 + TX + 1 <= W;

    // Unconditional clamped loads + deferred zero-select (a select
    // attached to each load makes hipcc emit a full vmcnt(0) drain per
    // load, serializing the HBM latency). The load and the store phase
    // are both free of control flow: a thread past the end of the plane
    // in the last round handles its previous round's element a second
    // time (same value to the same LDS address). With a per-thread
    // `break` in the store phase hipcc sinks each load into the
    // conditional block of its store, next to a vmcnt(0) — the loads
    // then fly over nothing.
    static_assert(SY * SX * C4N > 512 && SY * SX * C4N > (LV - 1) * 512, "");
    auto plane_idx = [&](int li) {
        const int idx = tid + li * 512;
        return idx < SY * SX * C4N ? idx : idx - 512;
    };
    auto plane_load = [&](int P, f32x4 (&vals)[LV], bool (&keep)[LV]) {
        const bool zin = P >= 0 && P < D;
        const bool interior = zin && xy_interior;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = plane_idx(li);
            const int c4 = idx % C4N;
            const int v = idx / C4N;
            const int gy = y0 + v / SX - 1;
            const int gx = x0 + v % SX - 1;
            const bool ok = zin && (interior ||
                                    (gy >= 0 && gy < H && gx >= 0 &&
                                     gx < W));
            keep[li] = ok;
            vals[li] = *reinterpret_cast<const f32x4*>(
                in + ((((long long)n * D + (zin ? P : 0)) * H +
                       (ok ? gy : 0)) * W + (ok ? gx : 0)) * C + c4 * 4);
        }
    };
    auto plane_store = [&](int P, const f32x4 (&vals)[LV],
                           const bool (&keep)[LV]) {
        const int slot = ((P + 1) % 3 + 3) % 3;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = plane_idx(li);
            const int c4 = idx % C4N;
            const int v = idx / C4N;
            *reinterpret_cast<f32x4*>(
                &ring[(slot * SY * SX + v) * PC + c4 * 4]) =
                keep[li] ? vals[li] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    {
        f32x4 wv[WL];
        bool wk[WL];
        f32x4 v0[LV], v1[LV];
        bool k0[LV], k1[LV];
        if (wvec) wall_load(wv, wk);  // one batch with the two planes
        plane_load(-1, v0, k0);
        plane_load(0, v1, k1);
        if (wvec) wall_store(wv, wk);
        plane_store(-1, v0, k0);
        plane_store(0, v1, k1);
    }
    __syncthreads();

    int tmy[M_TILES], tmx[M_TILES];
#pragma unroll
    for (int m = 0; m < M_TILES; ++m) {
        const int g = wave * M_TILES + m;
        tmx[m] = (g % XT) * 16;
        tmy[m] = g / XT;
    }
    const int a_row = lane & 15;
    const int a_k = lane >> 4;
    const int col16 = lane & 15;
    const int colj = lane & 15;
    const int rbase = (lane >> 4) * 4;

    // the lane's bias values never change over z: loaded once (clamped
    // address; lanes with j >= K store nothing)
    float bj[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        bj[t] = bias ? bias[min(j0 + t * 16 + colj, K - 1)] : 0.f;
    // block tiles: the lane's B column, and the output it finishes —
    // position pos4 of the m-tile, column J4 + 4 t + col4
    const int col4 = lane & 3;
    const int pos4 = ((lane >> 2) & 3) * 4 + (lane >> 4);
    float bj4[N4];
#pragma unroll
    for (int t = 0; t < NT4; ++t)
        bj4[t] = bias ? bias[J4 + t * 4 + col4] : 0.f;
    // The lane's index into the block wall, hidden from the optimizer:
    // folded into the 16-wide wall's address family, the block wall's
    // 243 NT4 read addresses lie past the 64 KB reach of a ds_read offset
    // from that base, and hipcc then keeps every one of them in a VGPR of
    // its own across the z loop (194 spills at C=36). Opaque, they share
    // one base register.
    int w4lane = W16 + a_k * 4 + col4;
    asm volatile("" : "+v"(w4lane));

    for (int z = 0; z < D; ++z) {
        // Two accumulator chains per m-tile: consecutive MFMAs on the
        // SAME accumulator pay the 40-cyc dependent latency against a
        // 32-cyc issue slot (PMC: 51.6% SQ_WAIT_INST_ANY with the naive
        // nt-outer order). kk-outer alternates the NT=2 accumulators
        // (bit-identical sums — each chain keeps its order); SPLIT
        // splits by kk parity into acc/acc2 (a benign reassociation,
        // folded in the epilogue). Each block tile has its own chain.
        f32x4 acc[M_TILES][NT];
        f32x4 acc2[M_TILES];
        f32x4 acc4[M_TILES][N4];
#pragma unroll
        for (int m = 0; m < M_TILES; ++m) {
            acc2[m] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[m][t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < N4; ++t)
                acc4[m][t] = {0.f, 0.f, 0.f, 0.f};
        }

        auto compute_dzi = [&](int dzi) {
            const int slot = ((z + dzi) % 3 + 3) % 3;  // plane z + dzi - 1
            const float* plane = &ring[slot * SY * SX * PC];
#pragma unroll
            for (int tl = 0; tl < 9; ++tl) {
                const int tap = dzi * 9 + tl;
                const int dy = tl / 3 - 1;
                const int dx = tl % 3 - 1;
                const float* arow[M_TILES];
#pragma unroll
                for (int m = 0; m < M_TILES; ++m) {
                    arow[m] = &plane[((1 + tmy[m] + dy) * SX +
                                      (1 + tmx[m] + dx)) * PC +
                                     a_row * PC + a_k];
                }
                const float* wblk = &wall[tap * NT * C * 16];
                const float* wblk4 = &wall[w4lane + tap * NT4 * C * 4];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    float a[M_TILES];
#pragma unroll
                    for (int m = 0; m < M_TILES; ++m)
                        a[m] = arow[m][kk * 4];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const float b =
                            wblk[(nt * C + kk * 4 + a_k) * 16 + col16];
#pragma unroll
                        for (int m = 0; m < M_TILES; ++m) {
                            f32x4& dst = (SPLIT && (kk & 1))
                                             ? acc2[m] : acc[m][nt];
                            dst = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                a[m], b, dst, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < NT4; ++t) {
                        const float b4 =
                            wblk4[(t * C + kk * 4) * 4];
#pragma unroll
                        for (int m = 0; m < M_TILES; ++m)
                            acc4[m][t] = __builtin_amdgcn_mfma_f32_4x4x1f32(
                                a[m], b4, acc4[m][t], 0, 0, 0);
                    }
                    // One scheduling group per step; LDS reads, VALU and
                    // SALU may cross (mask 0x106). Without it hipcc
                    // spills 8 VGPRs at C=36. In the first 18 taps each step's
                    // MFMAs stay together; behind the barrier the C=36
                    // launch still runs its 81 block MFMAs after the 81
                    // 16-wide ones and holds their A values (255 VGPRs,
                    // no spill, occupancy is 2 by LDS either way;
                    // profiles/kernel_resources_zring_blocks.txt).
                    if (NT4 > 0) __builtin_amdgcn_sched_barrier(0x106);
                }
            }
        };

        f32x4 vals[LV];
        bool keep[LV];
        // The sched_barriers pin the pipeline: without the first the
        // scheduler sinks the loads down to the store phase, without the
        // second it lifts the stores' zero-select (and its vmcnt(0)) up
        // to the loads.
        plane_load(z + 1, vals, keep);  // flies over the next 18 taps
        __builtin_amdgcn_sched_barrier(0);
        compute_dzi(0);
        compute_dzi(1);
        __builtin_amdgcn_sched_barrier(0);
        plane_store(z + 1, vals, keep);
        __syncthreads();

        // Residual reads, batched from clamped addresses and issued
        // BEFORE the last 9 taps so they land under those MFMAs. Nothing
        // else is in flight here: plane_store above waited for this z's
        // plane loads, and with them for every older store. (A load in
        // the store loop costs a vmcnt(0) drain each — loads and stores
        // share the counter, so a wait behind a pending store is also a
        // wait for that store's acknowledgement.)
        float rv[M_TILES][NT][4];
        float rv4[M_TILES][N4];
        if (res) {
#pragma unroll
            for (int m = 0; m < M_TILES; ++m) {
                const int gym = min(y0 + tmy[m], H - 1);
                const int gx4 = min(x0 + tmx[m] + pos4, W - 1);
#pragma unroll
                for (int t = 0; t < NT4; ++t)
                    rv4[m][t] = res[
                        ((((long long)n * D + z) * H + gym) * W + gx4) * K +
                        J4 + t * 4 + col4];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int jm = min(j0 + t * 16 + colj, K - 1);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int gxm = min(x0 + tmx[m] + rbase + r, W - 1);
                        rv[m][t][r] = res[
                            ((((long long)n * D + z) * H + gym) * W + gxm) *
                                K + jm];
                    }
                }
            }
        }
        compute_dzi(2);

        // Every output of this z is finished in registers first, so the
        // stores below go out back to back with no wait between them.
        // ELU is branch-free: expm1f of the value where it is not
        // positive (0 elsewhere; NaN stays NaN), then a select.
        float ov[M_TILES][NT][4];
#pragma unroll
        for (int m = 0; m < M_TILES; ++m) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[m][t][r] + bj[t];
                    if (NT == 1) v += acc2[m][r];
                    if (res) v += rv[m][t][r];
                    if (do_elu) {
                        const float e = expm1f(v > 0.f ? 0.f : v);
                        v = v > 0.f ? v : e;
                    }
                    ov[m][t][r] = v;
                }
            }
        }
        // Block tiles: every lane adds the four k-slices of all four rows
        // in the one order (s_q + s_q^2) + (s_q^1 + s_q^3), keeps the row
        // of its own k-slice index, then bias, residual, ELU as above.
        float ov4[M_TILES][N4];
#pragma unroll
        for (int m = 0; m < M_TILES; ++m) {
#pragma unroll
            for (int t = 0; t < NT4; ++t) {
                float v = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s = acc4[m][t][i];
                    s += __shfl_xor(s, 32);
                    s += __shfl_xor(s, 16);
                    v = a_k == i ? s : v;
                }
                v += bj4[t];
                if (res) v += rv4[m][t];
                if (do_elu) {
                    const float e = expm1f(v > 0.f ? 0.f : v);
                    v = v > 0.f ? v : e;
                }
                ov4[m][t] = v;
            }
        }
#pragma unroll
        for (int m = 0; m < M_TILES; ++m) {
            const int gy = y0 + tmy[m];
            if (gy >= H) continue;
            // four consecutive lanes write the 16 contiguous bytes of one
            // position's block-tile columns
            const int gx4 = x0 + tmx[m] + pos4;
#pragma unroll
            for (int t = 0; t < NT4; ++t) {
                if (gx4 >= W) continue;
                out[((((long long)n * D + z) * H + gy) * W + gx4) * K + J4 +
                    t * 4 + col4] = ov4[m][t];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int j = j0 + t * 16 + colj;
                if (j >= K) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gx = x0 + tmx[m] + rbase + r;
                    if (gx >= W) continue;
                    out[((((long long)n * D + z) * H + gy) * W + gx) * K +
                        j] = ov[m][t][r];
                }
            }
        }
    }
}

// C=48 persistent-z ring: the full 27-tap weight wall (82.9 KB per
// 16-wide K tile) no longer fits LDS beside the 3-plane ring (103.7 KB),
// so the wall is DOUBLE-BUFFERED per 9-tap dzi group (2 x 27.6 KB) and
// each group's stage overlaps the previous group's MFMAs. K covered by
// three j0 launches. Per z: 3 barriers; wall restage is ~3% of the z's
// MFMA time (weights come from L2 after the first z). Buffer parity is
// (3*z + dzi) % 2 — odd group count flips the pairing every z, and each
// write lands on a buffer whose last reader sat before the previous
// barrier (see the B1/B2/B3 comments).
template <int C, int K, int TY, int TX>
__global__ __launch_bounds__(512, 1) void k_conv3_zring_dw(
    const float* __restrict__ in, const float* __restrict__ wgt,
    const float* __restrict__ bias, const float* __restrict__ res,
    float* __restrict__ out, int N, int D, int H, int W, int do_elu,
    int j0) {
    // ring stride: C+2 when C%32==16 (48 -> 50; mod 32 = 18 keeps the
    // A reads bank-conflict-free) — the +4 pad of padc() would push the
    // ring + double wall 3.7 KB past the 160 KB LDS. Stride 50 dwords is
    // only 8-byte aligned, so the ring staging stores are b64.
    constexpr int PC = (C % 32 == 16) ? C + 2 : padc(C);
    constexpr int SX = TX + 2;
    constexpr int SY = TY + 2;
    constexpr int KK = C / 4;
    constexpr int NW = 8;
    constexpr int XT = TX / 16;
    constexpr int M_TILES = (TY * XT) / NW;
    constexpr int C4N = C / 4;
    constexpr int LV = (SY * SX * C4N + 511) / 512;
    static_assert((TY * XT) % NW == 0, "");

    __shared__ float ring[3 * SY * SX * PC];
    __shared__ float wall[2][9 * C * 16];

    const int n = blockIdx.z;
    const int y0 = blockIdx.y * TY;
    const int x0 = blockIdx.x * TX;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;

    // stage the 9-tap group g (taps 9g..9g+8) into wall[buf]
    auto wall_store = [&](int g, int buf) {
        for (int idx = tid; idx < 9 * C * 16; idx += 512) {
            const int j = idx & 15;
            const int c = (idx >> 4) % C;
            const int tl = (idx >> 4) / C;
            const int jg = j0 + j;
            wall[buf][idx] =
                jg < K ? wgt[((long long)(9 * g + tl) * C + c) * K + jg]
                       : 0.f;
        }
    };

    const bool xy_interior = y0 >= 1 && y0 + TY + 1 <= H && x0 >= 1 &&
                             x0 + TX + 1 <= W;
    auto plane_load = [&](int P, f32x4 (&vals)[LV]) {
        const bool zin = P >= 0 && P < D;
        const bool interior = zin && xy_interior;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = tid + li * 512;
            if (idx >= SY * SX * C4N) break;
            const int c4 = idx % C4N;
            const int v = idx / C4N;
            const int gy = y0 + v / SX - 1;
            const int gx = x0 + v % SX - 1;
            if (interior) {
                vals[li] = *reinterpret_cast<const f32x4*>(
                    in + ((((long long)n * D + P) * H + gy) * W + gx) * C +
                    c4 * 4);
            } else {
                const bool ok = zin && gy >= 0 && gy < H && gx >= 0 &&
                                gx < W;
                vals[li] = *reinterpret_cast<const f32x4*>(
                    in + ((((long long)n * D + (zin ? P : 0)) * H +
                           (ok ? gy : 0)) * W + (ok ? gx : 0)) * C +
                    c4 * 4);
                if (!ok) vals[li] = {0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    auto plane_store = [&](int P, const f32x4 (&vals)[LV]) {
        const int slot = ((P + 1) % 3 + 3) % 3;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = tid + li * 512;
            if (idx >= SY * SX * C4N) break;
            const int c4 = idx % C4N;
            const int v = idx / C4N;
            float* dst = &ring[(slot * SY * SX + v) * PC + c4 * 4];
            *reinterpret_cast<f32x2*>(dst) = f32x2{vals[li][0], vals[li][1]};
            *reinterpret_cast<f32x2*>(dst + 2) =
                f32x2{vals[li][2], vals[li][3]};
        }
    };

    {
        f32x4 v0[LV], v1[LV];
        plane_load(-1, v0);
        plane_load(0, v1);
        plane_store(-1, v0);
        plane_store(0, v1);
        wall_store(0, 0);  // g0 of z=0 -> buf (3*0+0)%2 = 0
    }
    __syncthreads();

    int tmy[M_TILES], tmx[M_TILES];
#pragma unroll
    for (int m = 0; m < M_TILES; ++m) {
        const int g = wave * M_TILES + m;
        tmx[m] = (g % XT) * 16;
        tmy[m] = g / XT;
    }
    const int a_row = lane & 15;
    const int a_k = lane >> 4;
    const int col16 = lane & 15;
    const int colj = lane & 15;
    const int rbase = (lane >> 4) * 4;

    for (int z = 0; z < D; ++z) {
        f32x4 acc[M_TILES];
#pragma unroll
        for (int m = 0; m < M_TILES; ++m)
            acc[m] = {0.f, 0.f, 0.f, 0.f};

        auto compute_dzi = [&](int dzi, int buf) {
            const int slot = ((z + dzi) % 3 + 3) % 3;
            const float* plane = &ring[slot * SY * SX * PC];
            const float* wb = wall[buf];
#pragma unroll
            for (int tl = 0; tl < 9; ++tl) {
                const int dy = tl / 3 - 1;
                const int dx = tl % 3 - 1;
                const float* arow[M_TILES];
#pragma unroll
                for (int m = 0; m < M_TILES; ++m) {
                    arow[m] = &plane[((1 + tmy[m] + dy) * SX +
                                      (1 + tmx[m] + dx)) * PC +
                                     a_row * PC + a_k];
                }
                const float* wblk = &wb[tl * C * 16];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const float b = wblk[(kk * 4 + a_k) * 16 + col16];
#pragma unroll
                    for (int m = 0; m < M_TILES; ++m) {
                        const float a = arow[m][kk * 4];
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            a, b, acc[m], 0, 0, 0);
                    }
                }
            }
        };

        const int p = (3 * z) % 2;  // buffer of this z's g0
        f32x4 vals[LV];
        plane_load(z + 1, vals);
        wall_store(1, 1 - p);      // g1 -> other buf (last read: g2 of z-1)
        compute_dzi(0, p);
        __syncthreads();           // B1: g1 visible; g0 buf free
        wall_store(2, p);          // g2 overwrites g0's buf
        compute_dzi(1, 1 - p);
        plane_store(z + 1, vals);
        __syncthreads();           // B2: g2 + plane z+1 visible; g1 buf free
        if (z + 1 < D)
            wall_store(0, 1 - p);  // next z's g0 -> (3(z+1))%2 == 1-p
        compute_dzi(2, p);

#pragma unroll
        for (int m = 0; m < M_TILES; ++m) {
            const int gy = y0 + tmy[m];
            if (gy >= H) continue;
            const int j = j0 + colj;
            if (j >= K) continue;
            const float bj = bias ? bias[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gx = x0 + tmx[m] + rbase + r;
                if (gx >= W) continue;
                long long o =
                    ((((long long)n * D + z) * H + gy) * W + gx) * K + j;
                float v = acc[m][r] + bj;
                if (res) v += res[o];
                if (do_elu) v = v > 0.f ? v : expm1f(v);
                out[o] = v;
            }
        }
        __syncthreads();           // B3: next z's g0 visible; g2 buf free
    }
}

}  // namespace

extern "C" int cfx_conv3_ndhwc_zring(cfx_ctx* ctx, const float* in,
                                     const float* wgt, const float* bias,
                                     const float* residual, float* out,
                                     int N, int D, int H, int W, int C,
                                     int K, int do_elu) {
    dim3 grid((W + 15) / 16, (H + 7) / 8, (unsigned)N);
    // float4 wall staging needs 16-byte-aligned weight rows; otherwise the
    // ring takes its scalar staging loop
    const int wvec =
        (reinterpret_cast<uintptr_t>(wgt) % 16 == 0 && K % 4 == 0) ? 1 : 0;
    double flops = 2.0 * 27.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV, flops, [&] {
        if (C == 28 && K == 28) {
            // wall holds both K tiles (96.8 KB + 60.5 KB ring). Three block
            // tiles for columns 16..27 instead of the second tile measured
            // slower (6.37 -> 6.61 ms)
            hipLaunchKernelGGL((k_conv3_zring_pl<28, 28, 8, 16, 2, 0, 0>),
                               grid, dim3(512), 0, ctx->stream, in, wgt, bias,
                               residual, out, N, D, H, W, do_elu, 0, wvec);
        } else if (C == 36 && K == 36) {
            // the wall beside the ring holds one 16-wide K tile, so two
            // launches: A = columns 0..15 plus 32..35 on a block tile out of
            // the same staged planes, B = columns 16..31. The input re-read
            // costs ~2x HBM traffic of a 113 MB activation per conv —
            // negligible next to the compute
            hipLaunchKernelGGL((k_conv3_zring_pl<36, 36, 8, 16, 1, 1, 32>),
                               grid, dim3(512), 0, ctx->stream, in, wgt, bias,
                               residual, out, N, D, H, W, do_elu, 0, wvec);
            hipLaunchKernelGGL((k_conv3_zring_pl<36, 36, 8, 16, 1, 0, 0>),
                               grid, dim3(512), 0, ctx->stream, in, wgt, bias,
                               residual, out, N, D, H, W, do_elu, 16, wvec);
        } else if (C == 48 && K == 48) {
            // double-buffered per-dzi weight wall (full wall no longer fits
            // beside the ring); one 16-wide K tile per launch
            for (int j0 = 0; j0 < 48; j0 += 16) {
                hipLaunchKernelGGL((k_conv3_zring_dw<48, 48, 8, 16>), grid,
                                   dim3(512), 0, ctx->stream, in, wgt, bias,
                                   residual, out, N, D, H, W, do_elu, j0);
            }
        } else {
            g_err = "cfx_conv3_ndhwc_zring: width not instantiated";
            return -1;
        }
        return 0;
    });
}

namespace {

// bf16 persistent-z ring (config-5 path): v_mfma_f32_32x32x16_bf16 — one
// 32-x by 32-channel D tile per wave, K-reduction 16 input channels per
// instruction, fragment layout probe-verified on hardware
// (tools/mfma_layout_probe.py): A[i=l&31][k=8*(l>>5)+e], B likewise, D as
// the f32 32x32 map. Activations ride the 3-plane LDS ring in [x][c]
// order (lane reads its 8-channel A fragment as one 16-byte ds_read; the
// per-x stride is padded to 40 elements so the 16-lane b128 groups land
// on distinct banks); the bf16 weight wall (27 taps x 32 j x padded c)
// stays LDS-resident for the whole workgroup. C is zero-padded to 32.
typedef __bf16 cfx_bf16;
typedef cfx_bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The C = K = 28 ring ("_a": two alternating accumulators, see the z
// loop). One barrier per z, software-pipelined like k_conv3_zring_pl,
// with the plane staging running one iteration ahead and a transposed
// wide-store epilogue.
template <int C, int K, int TY, int TX>
__global__ __launch_bounds__(512, 1) void k_conv3_zring_bf16_a(
    const cfx_bf16* __restrict__ in,    // (N, D, H, W, C)
    const cfx_bf16* __restrict__ wgt,   // (27, 32, 32): [tap][j][c], padded
    const float* __restrict__ bias,     // (K) f32
    const cfx_bf16* __restrict__ res,   // optional residual (out layout)
    cfx_bf16* __restrict__ out,         // (N, D, H, W, K)
    int N, int D, int H, int W, int do_elu) {
    constexpr int CP = 32;               // padded channel count
    constexpr int PCB = CP + 8;          // ring per-x stride (bank spread)
    constexpr int SX = TX + 2;
    constexpr int SY = TY + 2;
    constexpr int C4 = CP / 4;
    constexpr int LV = (SY * SX * C4 + 511) / 512;
    typedef cfx_bf16 bf16x4 __attribute__((ext_vector_type(4)));
    typedef cfx_bf16 bf16x8w __attribute__((ext_vector_type(8)));
    static_assert(C <= CP && K <= 32, "");

    __shared__ cfx_bf16 ring[3 * SY * SX * PCB];
    __shared__ cfx_bf16 wall[27 * 32 * PCB];
    // wave-private transpose scratch for the epilogue:
    // [wave][x-row 16][j 32] bf16 (1 KB per wave; no cross-wave sync)
    __shared__ cfx_bf16 oscr[8][16][32];

    const int n = blockIdx.z;
    const int y0 = blockIdx.y * TY;
    const int x0 = blockIdx.x * TX;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;           // 0..7 -> y row (TY == 8)
    const int lane = tid & 63;

    // weight wall, staged once: wall[(tap*32 + j)*PCB + c]
    for (int idx = tid; idx < 27 * 32 * CP; idx += 512) {
        const int c = idx % CP;
        const int j = (idx / CP) % 32;
        const int tap = idx / (CP * 32);
        wall[(tap * 32 + j) * PCB + c] = wgt[(tap * 32 + j) * 32 + c];
    }

    const bool xy_interior = y0 >= 1 && y0 + TY + 1 <= H && x0 >= 1 &&
                             x0 + TX + 1 <= W;

    // Staging is load-phase/store-phase with EXPLICIT register arrays and
    // unconditional loads from clamped addresses (any masked or pad lane
    // reads a safe in-bounds element); the zero-select runs in the store
    // phase, after the whole batch is in flight. A select attached to
    // each load, or a single dynamic loop, makes the compiler emit a full
    // vmcnt(0) drain per 8-byte load (~900 cy of HBM latency each,
    // serialized; the phase ablation priced it at ~2.6 ms of a 5.9 ms
    // launch).
    auto plane_load = [&](int P, bf16x4 (&vals)[LV], bool (&keep)[LV]) {
        const bool zin = P >= 0 && P < D;
        const bool interior = zin && xy_interior;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = min(tid + li * 512, SY * SX * C4 - 1);
            const int c4 = idx % C4;
            const int v = idx / C4;
            const int gy = y0 + v / SX - 1;
            const int gx = x0 + v % SX - 1;
            const bool cok = c4 * 4 < C;
            const bool ok = cok && zin &&
                            (interior || (gy >= 0 && gy < H && gx >= 0 &&
                                          gx < W));
            keep[li] = ok;
            vals[li] = *reinterpret_cast<const bf16x4*>(
                in + ((((long long)n * D + (zin ? P : 0)) * H +
                       (ok ? gy : 0)) * W + (ok ? gx : 0)) * C +
                (cok ? c4 * 4 : 0));
        }
    };
    auto plane_store = [&](int P, const bf16x4 (&vals)[LV],
                           const bool (&keep)[LV]) {
        const int slot = ((P + 1) % 3 + 3) % 3;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = tid + li * 512;
            if (idx >= SY * SX * C4) break;
            const int c4 = idx % C4;
            const int v = idx / C4;
            *reinterpret_cast<bf16x4*>(
                &ring[((slot * SY + v / SX) * SX + v % SX) * PCB +
                      c4 * 4]) = keep[li] ? vals[li] : bf16x4{};
        }
    };

    {
        bf16x4 v0[LV], v1[LV];
        bool k0[LV], k1[LV];
        plane_load(-1, v0, k0);
        plane_load(0, v1, k1);
        plane_store(-1, v0, k0);
        plane_store(0, v1, k1);
    }
    __syncthreads();
    // One-iteration-ahead staging: plane z+1 is loaded during iteration
    // z-1, so the store in iteration z never waits on its own loads
    // (the phase timing showed 24% of the z period in store+barrier)
    bf16x4 va[LV];
    bool ka[LV];
    plane_load(1, va, ka);

    const int ax = lane & 31;            // A row (x), B col (j)
    const int khalf = (lane >> 5) * 8;   // this lane's k sub-range base

    for (int z = 0; z < D; ++z) {
        // TWO alternating accumulators: anything issued between two MFMAs
        // on the SAME accumulator costs a +43-cycle cliff (microarch
        // guide, per-instruction constants) and this loop has 2 LDS reads
        // + loop VALU per MFMA; alternating pairs makes consecutive MFMAs
        // hit different accumulators (~6 cyc/state instead). Accumulation
        // order is evens + odds.
        f32x16 accA = {};
        f32x16 accB = {};
        // Fragment addressing for the flat pair pipeline (pair p: tap
        // p>>1, kk p&1), split at pair 36 around the plane barrier.
        // Explicit prefetch at distance PD = 4: the compiler's natural
        // schedule issues a pair's ds_reads only ~1 MFMA before their
        // s_waitcnt, so every tap parks for the LDS latency (PMC: 67%
        // SQ_WAIT_ANY). With 4 MFMAs in flight (~128 cyc) the read
        // latency is covered and the waitcnts become lgkmcnt(6) partial
        // waits; the sched_barriers keep the compiler from undoing it.
        const cfx_bf16* planes[3];
#pragma unroll
        for (int dzi = 0; dzi < 3; ++dzi)
            planes[dzi] = &ring[(((z + dzi) % 3 + 3) % 3) * SY * SX * PCB];
        auto addrA = [&](int p) {
            const int tap = p >> 1, kk = p & 1;
            const int dzi = tap / 9, tl = tap % 9;
            const int dy = tl / 3 - 1, dx = tl % 3 - 1;
            return reinterpret_cast<const bf16x8*>(
                &planes[dzi][((1 + wave + dy) * SX + (1 + dx) + ax) * PCB +
                             khalf + kk * 16]);
        };
        auto addrB = [&](int p) {
            const int tap = p >> 1, kk = p & 1;
            return reinterpret_cast<const bf16x8*>(
                &wall[(tap * 32 + ax) * PCB + khalf + kk * 16]);
        };
        constexpr int PD = 4;

        bf16x4 vals[LV];
        bool keep[LV];
        plane_load(z + 2, vals, keep);  // lands during NEXT iteration
        {
            bf16x8 abuf[PD], bbuf[PD];
#pragma unroll
            for (int p = 0; p < PD; ++p) {
                abuf[p] = *addrA(p);
                bbuf[p] = *addrB(p);
            }
#pragma unroll
            for (int p = 0; p < 36; ++p) {  // dzi 0,1: planes z-1, z
                const int si = p % PD;
                if (p & 1)
                    accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accB, 0, 0, 0);
                else
                    accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accA, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (p + PD < 36) {
                    abuf[si] = *addrA(p + PD);
                    bbuf[si] = *addrB(p + PD);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            plane_store(z + 1, va, ka);
            __syncthreads();
#pragma unroll
            for (int p = 36; p < 36 + PD; ++p) {
                abuf[p % PD] = *addrA(p);
                bbuf[p % PD] = *addrB(p);
            }
#pragma unroll
            for (int p = 36; p < 54; ++p) {  // dzi 2: plane z + 1
                const int si = p % PD;
                if (p & 1)
                    accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accB, 0, 0, 0);
                else
                    accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accA, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (p + PD < 54) {
                    abuf[si] = *addrA(p + PD);
                    bbuf[si] = *addrB(p + PD);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

#pragma unroll
        for (int li = 0; li < LV; ++li) {
            va[li] = vals[li];
            ka[li] = keep[li];
        }
        const f32x16 acc = accA + accB;
        // Transposed epilogue: the MFMA's j-per-lane layout would store
        // 16 scattered 2-byte elements per lane per z; those 128 store
        // instructions per CU per z measured as 40% of the launch
        // (DESIGN §10-r2). Bounce the 32x32 tile through wave-private
        // LDS in two 16-row halves (the full tile would need 16 KB of
        // scratch and bust the 160 KB LDS budget) and store x-major: one
        // coalesced b128/b64 store per lane per half. Residual reads
        // ride the same wide path; (acc+bias) rounds through bf16 before
        // the res add.
        const int gy = y0 + wave;
        const int j = lane & 31;
        const float bj = (bias && j < K) ? bias[j] : 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int r = 8 * h; r < 8 * h + 8; ++r) {
                const int row = (r & 3) + 8 * ((r >> 2) & 1) +
                                4 * (lane >> 5);
                oscr[wave][row][j] = (cfx_bf16)(acc[r] + bj);
            }
            const int xr = lane >> 2;       // x row 0..15 in half
            const int ch = lane & 3;        // 16-byte chunk 0..3
            const int gx = x0 + 16 * h + xr;
            if (gy < H && gx < W) {
                const int j0 = ch * 8;
                long long o = ((((long long)n * D + z) * H + gy) *
                               W + gx) * K + j0;
                if (j0 + 8 <= K) {
                    bf16x8w v = *reinterpret_cast<const bf16x8w*>(
                        &oscr[wave][xr][j0]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float t = (float)v[e];
                        if (res) t += (float)res[o + e];
                        if (do_elu) t = t > 0.f ? t : expm1f(t);
                        v[e] = (cfx_bf16)t;
                    }
                    *reinterpret_cast<bf16x8w*>(out + o) = v;
                } else if (j0 < K) {        // tail chunk (K=28)
                    bf16x4 v = *reinterpret_cast<const bf16x4*>(
                        &oscr[wave][xr][j0]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = (float)v[e];
                        if (res) t += (float)res[o + e];
                        if (do_elu) t = t > 0.f ? t : expm1f(t);
                        v[e] = (cfx_bf16)t;
                    }
                    *reinterpret_cast<bf16x4*>(out + o) = v;
                }
            }
        }
    }
}

// Sliced bf16 ring: the ring above (staging not run ahead) generalized
// to a c-slice [c0, c0+CL)
// of a wider channel dimension (runtime stride CS) and a j-tile
// [j0, j0+32) of a wider K (runtime stride KS). Widths 36 and 48 run as
// four launches — (c 0..31, CPV=32) + (c 32.., CPV=16), each for j-tiles
// j0=0 and j0=32 — reusing the PCB=CP+8 LDS layout whose strides (40/24
// elements) are the measured conflict-free ones. The second c-half launch
// chains through `res` = its own output (partial sums round through bf16
// between halves; bias/ELU apply only on the final half). Weight pack:
// [27][64][48] zero-padded, [tap][j][c].
template <int CPV, int TY, int TX>
__global__ __launch_bounds__(512, 1) void k_conv3_zring_bf16_s(
    const cfx_bf16* __restrict__ in, const cfx_bf16* __restrict__ wgt,
    const float* __restrict__ bias, const cfx_bf16* __restrict__ res,
    cfx_bf16* __restrict__ out, int N, int D, int H, int W, int CS,
    int CL, int c0, int KS, int Ktot, int j0, int do_elu) {
    constexpr int CP = CPV;
    constexpr int PCB = CP + 8;
    constexpr int SX = TX + 2;
    constexpr int SY = TY + 2;
    constexpr int KK = CP / 16;
    constexpr int C4 = CP / 4;
    constexpr int LV = (SY * SX * C4 + 511) / 512;
    typedef cfx_bf16 bf16x4 __attribute__((ext_vector_type(4)));
    constexpr int WPK = 64;  // weight pack j rows
    constexpr int WPC = 48;  // weight pack c width

    __shared__ cfx_bf16 ring[3 * SY * SX * PCB];
    __shared__ cfx_bf16 wall[27 * 32 * PCB];
    __shared__ cfx_bf16 oscr[8][16][32];  // transposed-epilogue scratch

    const int n = blockIdx.z;
    const int y0 = blockIdx.y * TY;
    const int x0 = blockIdx.x * TX;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;

    for (int idx = tid; idx < 27 * 32 * CP; idx += 512) {
        const int c = idx % CP;
        const int j = (idx / CP) % 32;
        const int tap = idx / (CP * 32);
        wall[(tap * 32 + j) * PCB + c] =
            wgt[(tap * WPK + j0 + j) * WPC + c0 + c];
    }

    const bool xy_interior = y0 >= 1 && y0 + TY + 1 <= H && x0 >= 1 &&
                             x0 + TX + 1 <= W;

    auto plane_load = [&](int P, bf16x4 (&vals)[LV], bool (&keep)[LV]) {
        const bool zin = P >= 0 && P < D;
        const bool interior = zin && xy_interior;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = min(tid + li * 512, SY * SX * C4 - 1);
            const int c4 = idx % C4;
            const int v = idx / C4;
            const int gy = y0 + v / SX - 1;
            const int gx = x0 + v % SX - 1;
            const bool cok = c4 * 4 < CL;
            const bool ok = cok && zin &&
                            (interior || (gy >= 0 && gy < H && gx >= 0 &&
                                          gx < W));
            keep[li] = ok;
            vals[li] = *reinterpret_cast<const bf16x4*>(
                in + (((long long)n * D + (zin ? P : 0)) * H +
                      (ok ? gy : 0)) * (long long)W * CS +
                (ok ? gx : 0) * (long long)CS + c0 + (cok ? c4 * 4 : 0));
        }
    };
    auto plane_store = [&](int P, const bf16x4 (&vals)[LV],
                           const bool (&keep)[LV]) {
        const int slot = ((P + 1) % 3 + 3) % 3;
#pragma unroll
        for (int li = 0; li < LV; ++li) {
            const int idx = tid + li * 512;
            if (idx >= SY * SX * C4) break;
            const int c4 = idx % C4;
            const int v = idx / C4;
            *reinterpret_cast<bf16x4*>(
                &ring[((slot * SY + v / SX) * SX + v % SX) * PCB +
                      c4 * 4]) = keep[li] ? vals[li] : bf16x4{};
        }
    };

    {
        bf16x4 v0[LV], v1[LV];
        bool k0[LV], k1[LV];
        plane_load(-1, v0, k0);
        plane_load(0, v1, k1);
        plane_store(-1, v0, k0);
        plane_store(0, v1, k1);
    }
    __syncthreads();

    const int ax = lane & 31;
    const int khalf = (lane >> 5) * 8;

    for (int z = 0; z < D; ++z) {
        f32x16 acc = {};   // even pairs; accB odd (same-acc-cliff dodge,
        f32x16 accB = {};  // see k_conv3_zring_bf16_a)
        const cfx_bf16* planes[3];
#pragma unroll
        for (int dzi = 0; dzi < 3; ++dzi)
            planes[dzi] = &ring[(((z + dzi) % 3 + 3) % 3) * SY * SX * PCB];
        auto addrA = [&](int p) {
            const int tap = p / KK, kk = p % KK;
            const int dzi = tap / 9, tl = tap % 9;
            const int dy = tl / 3 - 1, dx = tl % 3 - 1;
            return reinterpret_cast<const bf16x8*>(
                &planes[dzi][((1 + wave + dy) * SX + (1 + dx) + ax) * PCB +
                             khalf + kk * 16]);
        };
        auto addrB = [&](int p) {
            const int tap = p / KK, kk = p % KK;
            return reinterpret_cast<const bf16x8*>(
                &wall[(tap * 32 + ax) * PCB + khalf + kk * 16]);
        };
        constexpr int PD = 4;
        constexpr int NP1 = 18 * KK;  // dzi 0,1: planes z-1, z
        constexpr int NP2 = 27 * KK;

        bf16x4 vals[LV];
        bool keep[LV];
        plane_load(z + 1, vals, keep);
        {
            bf16x8 abuf[PD], bbuf[PD];
#pragma unroll
            for (int p = 0; p < PD; ++p) {
                abuf[p] = *addrA(p);
                bbuf[p] = *addrB(p);
            }
#pragma unroll
            for (int p = 0; p < NP1; ++p) {
                const int si = p % PD;
                if (p & 1)
                    accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accB, 0, 0, 0);
                else
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (p + PD < NP1) {
                    abuf[si] = *addrA(p + PD);
                    bbuf[si] = *addrB(p + PD);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            plane_store(z + 1, vals, keep);
            __syncthreads();
#pragma unroll
            for (int p = NP1; p < NP1 + PD; ++p) {
                abuf[p % PD] = *addrA(p);
                bbuf[p % PD] = *addrB(p);
            }
#pragma unroll
            for (int p = NP1; p < NP2; ++p) {
                const int si = p % PD;
                if (p & 1)
                    accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], accB, 0, 0, 0);
                else
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        abuf[si], bbuf[si], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (p + PD < NP2) {
                    abuf[si] = *addrA(p + PD);
                    bbuf[si] = *addrB(p + PD);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        acc = acc + accB;
        // transposed wide-store epilogue (see k_conv3_zring_bf16_a):
        // two 16-row halves through wave-private LDS, one
        // coalesced b128/b64 store per lane per half. rem per 8-j chunk
        // is always 8, 4 or <=0 for K in {28, 36, 48}.
        const int gy = y0 + wave;
        const int j = lane & 31;
        if (gy < H) {
            const float bj =
                (bias && j0 + j < Ktot) ? bias[j0 + j] : 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int r = 8 * h; r < 8 * h + 8; ++r) {
                    const int row = (r & 3) + 8 * ((r >> 2) & 1) +
                                    4 * (lane >> 5);
                    oscr[wave][row][j] = (cfx_bf16)(acc[r] + bj);
                }
                const int xr = lane >> 2;
                const int ch = lane & 3;
                const int gx = x0 + 16 * h + xr;
                const int rem = Ktot - j0 - ch * 8;
                if (gx < W && rem >= 4) {
                    const int j0c = ch * 8;
                    long long o = (((long long)n * D + z) * H + gy) *
                                      (long long)W * KS +
                                  (long long)gx * KS + j0 + j0c;
                    typedef cfx_bf16 bf16x8s
                        __attribute__((ext_vector_type(8)));
                    if (rem >= 8) {
                        bf16x8s v = *reinterpret_cast<const bf16x8s*>(
                            &oscr[wave][xr][j0c]);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float t = (float)v[e];
                            if (res) t += (float)res[o + e];
                            if (do_elu) t = t > 0.f ? t : expm1f(t);
                            v[e] = (cfx_bf16)t;
                        }
                        *reinterpret_cast<bf16x8s*>(out + o) = v;
                    } else {
                        bf16x4 v = *reinterpret_cast<const bf16x4*>(
                            &oscr[wave][xr][j0c]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float t = (float)v[e];
                            if (res) t += (float)res[o + e];
                            if (do_elu) t = t > 0.f ? t : expm1f(t);
                            v[e] = (cfx_bf16)t;
                        }
                        *reinterpret_cast<bf16x4*>(out + o) = v;
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" int cfx_conv3_ndhwc_bf16(cfx_ctx* ctx, const void* in,
                                    const void* wgt, const float* bias,
                                    const void* residual, void* out, int N,
                                    int D, int H, int W, int C, int K,
                                    int do_elu) {
    const bool sliced = (C == 36 && K == 36) || (C == 48 && K == 48);
    if (!sliced && (C != 28 || K != 28)) {
        g_err = "cfx_conv3_ndhwc_bf16: only C == K == 28/36/48 instantiated";
        return -1;
    }
    dim3 grid((W + 31) / 32, (H + 7) / 8, (unsigned)N);
    double flops = 2.0 * 27.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV, flops, [&] {
        if (sliced) {
            // (c-half, j-tile) x 4 launches; wgt pack is [27][64][48]
            // zero-padded. Bias/ELU only on the final c-half, which chains
            // through res = its own output.
            const int CL2 = C - 32;
            for (int j0 = 0; j0 < K; j0 += 32) {
                hipLaunchKernelGGL((k_conv3_zring_bf16_s<32, 8, 32>), grid,
                                   dim3(512), 0, ctx->stream,
                                   (const cfx_bf16*)in, (const cfx_bf16*)wgt,
                                   nullptr, (const cfx_bf16*)residual,
                                   (cfx_bf16*)out, N, D, H, W, C, 32, 0, K,
                                   K, j0, 0);
                hipLaunchKernelGGL((k_conv3_zring_bf16_s<16, 8, 32>), grid,
                                   dim3(512), 0, ctx->stream,
                                   (const cfx_bf16*)in, (const cfx_bf16*)wgt,
                                   bias, (const cfx_bf16*)out,
                                   (cfx_bf16*)out, N, D, H, W, C, CL2, 32, K,
                                   K, j0, do_elu);
            }
        } else {
            hipLaunchKernelGGL((k_conv3_zring_bf16_a<28, 28, 8, 32>), grid,
                               dim3(512), 0, ctx->stream,
                               (const cfx_bf16*)in, (const cfx_bf16*)wgt,
                               bias, (const cfx_bf16*)residual,
                               (cfx_bf16*)out, N, D, H, W, do_elu);
        }
        return 0;
    });
}
