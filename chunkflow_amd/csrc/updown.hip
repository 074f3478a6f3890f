// Up/down-sampling convolutions of the RSUNet encoder/decoder on gfx950.
//
// The reference runs these through torch -> MIOpen (ConvTranspose3d /
// strided Conv3d). The (1,2,2)-kernel, (1,2,2)-stride shapes are pure
// HBM-streaming work (a C-vector read + K-vector write per spatial
// position; no tap overlap), and MIOpen's bf16 bwd_data implicit GEMM is
// far off that roofline on the big up-conv (measured 8.0 ms vs ~0.2 ms
// algorithmic at 36->28 x 128^2, profiles/updown_probe_r02.json). The
// k_upconv2 / k_downconv2 kernels are VALU streams: input row and weights
// staged to LDS in
// batched coalesced loads (a per-load global read next to its use costs a
// full vmcnt drain — the round-1 staging lesson), per-thread accumulators
// over 8 x-positions so each weight vector is read once per c. The f32
// up-conv of MFMA-shaped widths and the 28 -> 3 output conv run on the f32
// matrix cores instead (k_upconv2_mfma, k_conv155_out_mfma below), and so
// does the 1 -> 28 input conv (k_conv155_in_mfma).
//
// Layouts: NDHWC (channels_last_3d); weights packed
// [parity q=(py<<1)|px][C][K] (stored in LDS as [c][k][q] float4 so one
// ds_read_b128 serves all four parities). bias f32 (may be NULL).
// No activation (RSUNet applies none here). f32 accumulation.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>

#include "cfx_internal.h"

namespace {

typedef __hip_bfloat16 cfx_bf16;

template <typename T>
__device__ __forceinline__ float ldf(const T* p);
template <>
__device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ldf<cfx_bf16>(const cfx_bf16* p) {
    return __bfloat162float(*p);
}
__device__ __forceinline__ float cvf(float v) { return v; }
__device__ __forceinline__ float cvf(cfx_bf16 v) {
    return __bfloat162float(v);
}

// 4-wide raw vector per dtype (__hip_bfloat16 is a struct, so its raw
// bits travel as ushort lanes)
template <typename T>
struct vec4;
template <>
struct vec4<float> {
    typedef float type __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float get(type v, int i) {
        return v[i];
    }
};
template <>
struct vec4<cfx_bf16> {
    typedef unsigned short type __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float get(type v, int i) {
        return __bfloat162float(
            __hip_bfloat16(__hip_bfloat16_raw{(unsigned short)v[i]}));
    }
};
template <typename T>
__device__ __forceinline__ void stf(T* p, float v);
template <>
__device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void stf<cfx_bf16>(cfx_bf16* p, float v) {
    *p = __float2bfloat16(v);
}

__device__ __forceinline__ unsigned short bf16_bits(float v) {
    return ((__hip_bfloat16_raw)__float2bfloat16(v)).x;
}

// cooperative stage of `rows` input rows (each `xn` positions x C
// channels, row r at in + row_off[r]) into s_in[r * xn * CPAD + x * CPAD
// + c] as f32, batched so the loads pipeline (no per-load drain).
template <typename T>
__device__ __forceinline__ void stage_rows(
    float* s_in, const T* in, const long long* row_off, int rows, int xn,
    int xvalid, int C, int CPAD, int tid, int nthreads) {
    const int total = rows * xn * C;
    for (int idx = tid; idx < total; idx += nthreads) {
        const int c = idx % C;
        const int x = (idx / C) % xn;
        const int r = idx / (C * xn);
        const float v = x < xvalid
                            ? ldf(&in[row_off[r] + (long long)x * C + c])
                            : 0.f;
        s_in[(r * xn + x) * CPAD + c] = v;
    }
}

// ---- transposed conv (1,2,2), stride (1,2,2) ------------------------------
// out[n, z, 2y+py, 2x+px, k] = bias[k] + sum_c in[n, z, y, x, c] * w[q][c][k]
// One workgroup: one (n, z, y) input row, XI input x positions, all K.
// 256 threads = 8 pos-slots x 32 k-slots; each thread accumulates XI/8
// x-positions x 4 parities so w4 is read once per (c, k).
template <typename T, int XI>
__global__ __launch_bounds__(256, 2) void k_upconv2(
    const T* __restrict__ in, const T* __restrict__ wgt,
    const float* __restrict__ bias, T* __restrict__ out, int N, int D,
    int H, int W, int C, int K) {
    constexpr int PX = XI / 8;  // x-positions per thread
    extern __shared__ float smem[];
    float* s_w = smem;                    // [C][K][4]
    float* s_in = smem + C * K * 4;       // [XI][CPAD]
    const int CPAD = C | 1;
    const int tid = threadIdx.x;
    const int kslot = tid & 31;
    const int pslot = tid >> 5;

    for (int idx = tid; idx < C * K * 4; idx += 256) {
        const int q = idx & 3;
        const int k = (idx >> 2) % K;
        const int c = (idx >> 2) / K;
        s_w[(c * K + k) * 4 + q] = ldf(&wgt[(q * C + c) * K + k]);
    }

    const int nz = blockIdx.z;           // n * D + z
    const int y = blockIdx.y;
    const int x0 = blockIdx.x * XI;
    const int xvalid = min(XI, W - x0);
    long long row_off[1] = {((((long long)nz * H) + y) * W + x0) * C};
    stage_rows(s_in, in, row_off, 1, XI, xvalid, C, CPAD, tid, 256);
    __syncthreads();

    const long long out_base =
        ((((long long)nz * 2 * H) + 2 * y) * 2 * W) * K;

    for (int k = kslot; k < K; k += 32) {
        const float bj = bias ? bias[k] : 0.f;
        float acc[PX][4];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = bj;
        for (int c = 0; c < C; ++c) {
            const float4 w4 =
                *reinterpret_cast<const float4*>(&s_w[(c * K + k) * 4]);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const float v = s_in[(pslot + p * 8) * CPAD + c];
                acc[p][0] += v * w4.x;
                acc[p][1] += v * w4.y;
                acc[p][2] += v * w4.z;
                acc[p][3] += v * w4.w;
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int xi = x0 + pslot + p * 8;
            if (xi >= W) continue;
            T* op = out + out_base + (long long)2 * xi * K + k;
            stf(op, acc[p][0]);
            stf(op + K, acc[p][1]);
            stf(op + (long long)2 * W * K, acc[p][2]);
            stf(op + (long long)2 * W * K + K, acc[p][3]);
        }
    }
}

// ---- transposed conv (1,2,2) on the f32 MFMA, optional fused skip-add -----
// out[n, z, 2y+py, 2x+px, k] = (bias[k] + sum_c in[n,z,y,x,c] * w[q][c][k])
//                              (+ skip[n, z, 2y+py, 2x+px, k])
// k_upconv2 above is LDS-bound (9 LDS reads per 32 FMAs), restages the
// whole weight table for every 64 input positions and stores single
// dwords. Here the op is the GEMM it is: per input position
//   out4K[q*K + k] = sum_c in[c] * w[q][c][k]
// with M = 16 input x positions (one tile), N = 4K = NT tiles of 16 and
// C/4 steps of v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate, exact: an
// fmaf chain over c in natural order that starts from the bias).
//
// One wave owns a tile; a workgroup of UM_NW waves stages the B fragments
// to LDS once ([step][tile][lane], one conflict-free ds_read_b32 per MFMA)
// and its waves then walk tiles grid-stride with no further barrier.
// A fragments come straight from global (lane (i, kk) reads
// in[x0+i][4s+kk]; the C/4 loads of a tile cover its contiguous 16*C
// floats). The accumulators leave through a wave-private LDS bounce
// [16 positions][4K + 4]: for a parity row py the tile's outputs are ONE
// contiguous run of 32K floats in output row 2y+py (position i holds the
// 2K floats (px, k) at bounce[i][py*2K ..]), so `out` and `skip` move as
// 16-byte accesses, K/4 per lane per tile. The +4 row pad spreads the
// accumulator's four row groups over the banks.
//
// Memory pipeline: a tile's skip loads and the NEXT tile's A loads are
// issued as one batch, from clamped addresses and with no branch around
// them, before the tile's MFMAs; they are the newest entries of vmcnt, so
// the MFMAs wait only for A values loaded a tile earlier and the epilogue's
// wait for the skip values counts the A prefetch behind them, never a
// drain (loads and stores share vmcnt; conv.hip's z-ring epilogue records
// the lesson). Partial tiles select at the store. The skip add is the last
// f32 add on the finished value, so the fused call equals the unfused
// kernel + a separate add bit for bit.

// waves per workgroup, one per SIMD. Workgroups pack onto a CU as
// registers and LDS allow: the 36 -> 28 kernel with skip (220 VGPRs +
// AGPRs, 46 KB) runs two, i.e. 2 waves per SIMD, which with the loads
// issued a phase ahead reaches 5.6 TB/s (profiles/upskip_probe.json)
constexpr int UM_NW = 4;

typedef float um_f32x4 __attribute__((ext_vector_type(4)));

template <int NT, bool SKIP>  // K = 4 * NT
__global__ __launch_bounds__(UM_NW * 64) void k_upconv2_mfma(
    const float* __restrict__ in, const float* __restrict__ wgt,
    const float* __restrict__ bias, const float* __restrict__ skip,
    float* __restrict__ out, int W, int C, int xtiles, int ntiles) {
    constexpr int K = 4 * NT;
    constexpr int N4 = 4 * K;     // GEMM N
    constexpr int BS = N4 + 4;    // bounce row stride, dwords
    constexpr int RUN4 = 2 * NT;  // 16-byte pieces per position per py
    extern __shared__ __attribute__((aligned(16))) float um_smem[];
    const int S = C >> 2;         // MFMA steps
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* s_w = um_smem;                               // [S][NT][64]
    float* s_b = um_smem + C * N4 + wave * (16 * BS);   // [16][BS]

    // B[k = lane>>4][j = lane&15] of (step s, tile t)
    for (int idx = tid; idx < C * N4; idx += UM_NW * 64) {
        const int l = idx & 63;
        const int st = idx >> 6;
        const int t = st % NT;
        const int s = st / NT;
        const int c = 4 * s + (l >> 4);
        const int col = 16 * t + (l & 15);
        const int q = col / K;
        s_w[idx] = wgt[(q * C + c) * K + (col - q * K)];
    }
    __syncthreads();

    const int ai = lane & 15;   // A row / D column
    const int akk = lane >> 4;  // A k / D row group
    float bj[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        bj[t] = bias ? bias[(16 * t + ai) % K] : 0.f;

    // epilogue piece `it` of this lane: f = it*64 + lane over
    // [py][position i][RUN4 pieces]
    auto piece = [&](int it, int& py, int& i, int& j4) {
        const int f = it * 64 + lane;
        py = f >= 16 * RUN4;
        const int rem = f - py * (16 * RUN4);
        i = rem / RUN4;
        j4 = rem - i * RUN4;
    };
    // global loads, branch-free, 32-bit lane offsets on wave-uniform tile
    // bases: the A fragments of a tile ...
    auto a_loads = [&](int tile, float (&a)[16]) {
        const int xt = tile % xtiles;
        const long long row = tile / xtiles;  // (n*D + z)*H + y
        const int x0 = xt * 16;
        const int ilast = min(16, W - x0) - 1;
        const float* ip = in + (row * W + x0) * C;
        const unsigned ao = min(ai, ilast) * C + akk;
#pragma unroll
        for (int s = 0; s < 16; ++s) a[s] = ip[ao + 4u * min(s, S - 1)];
    };
    // ... and its skip values, in the epilogue's piece order
    auto skip_loads = [&](int tile, um_f32x4 (&sv)[NT]) {
        const int xt = tile % xtiles;
        const long long row = tile / xtiles;
        const int x0 = xt * 16;
        const int ilast = min(16, W - x0) - 1;
        const float* sp = skip + (2 * row * 2 * W + 2 * x0) * K;
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            int py, i, j4;
            piece(it, py, i, j4);
            const unsigned so =
                py * (2 * W * K) + min(i, ilast) * (2 * K) + 4 * j4;
            sv[it] = *reinterpret_cast<const um_f32x4*>(sp + so);
        }
    };

    // one tile: its skip loads and the next tile's A loads fly over the
    // MFMAs on `a`
    auto do_tile = [&](int tile, int next, const float (&a)[16],
                       float (&a2)[16]) {
        um_f32x4 sv[NT];
        if (SKIP) skip_loads(tile, sv);
        a_loads(next, a2);
        __builtin_amdgcn_sched_barrier(0);
        um_f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            acc[t] = um_f32x4{bj[t], bj[t], bj[t], bj[t]};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (s >= S) break;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    a[s], s_w[(s * NT + t) * 64 + lane], acc[t], 0, 0, 0);
        }
        // D[row = akk*4 + r][col = ai] -> bounce[position][q*K + k]
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s_b[(akk * 4 + r) * BS + 16 * t + ai] = acc[t][r];
        __builtin_amdgcn_wave_barrier();

        const int xt = tile % xtiles;
        const long long row = tile / xtiles;
        const int x0 = xt * 16;
        const int nvalid = min(16, W - x0);
        float* op = out + (2 * row * 2 * W + 2 * x0) * K;
        // every output finished in registers first, then the stores go
        // out back to back
        um_f32x4 v[NT];
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            int py, i, j4;
            piece(it, py, i, j4);
            v[it] = *reinterpret_cast<const um_f32x4*>(
                &s_b[i * BS + py * (2 * K) + 4 * j4]);
            if (SKIP) v[it] += sv[it];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            int py, i, j4;
            piece(it, py, i, j4);
            const unsigned oo = py * (2 * W * K) + i * (2 * K) + 4 * j4;
            if (nvalid == 16 || i < nvalid)
                *reinterpret_cast<um_f32x4*>(op + oo) = v[it];
        }
        __builtin_amdgcn_wave_barrier();  // bounce is rewritten next tile
    };

    // two tiles per trip, the A register sets swapping roles (a copy at
    // the loop end would wait for the prefetch it copies)
    const int stride = gridDim.x * UM_NW;
    int tile = blockIdx.x * UM_NW + wave;
    if (tile >= ntiles) return;
    float a0[16], a1[16];
    a_loads(tile, a0);
    while (true) {
        do_tile(tile, min(tile + stride, ntiles - 1), a0, a1);
        tile += stride;
        if (tile >= ntiles) break;
        do_tile(tile, min(tile + stride, ntiles - 1), a1, a0);
        tile += stride;
        if (tile >= ntiles) break;
    }
}

// ---- down conv (1,2,2), stride (1,2,2) ------------------------------------
// out[n, z, y, x, k] = bias[k] + sum_q sum_c in[n, z, 2y+qy, 2x+qx, c] *
//                      w[q][c][k];  H, W are INPUT dims (out H/2 x W/2).
template <typename T, int XO>
__global__ __launch_bounds__(256, 2) void k_downconv2(
    const T* __restrict__ in, const T* __restrict__ wgt,
    const float* __restrict__ bias, T* __restrict__ out, int N, int D,
    int H, int W, int C, int K) {
    constexpr int PX = XO / 8;
    extern __shared__ float smem[];
    float* s_w = smem;                       // [C][K][4]
    float* s_in = smem + C * K * 4;          // [2 rows][2*XO][CPAD]
    const int CPAD = C | 1;
    const int tid = threadIdx.x;
    const int kslot = tid & 31;
    const int pslot = tid >> 5;
    const int HO = H >> 1, WO = W >> 1;

    for (int idx = tid; idx < C * K * 4; idx += 256) {
        const int q = idx & 3;
        const int k = (idx >> 2) % K;
        const int c = (idx >> 2) / K;
        s_w[(c * K + k) * 4 + q] = ldf(&wgt[(q * C + c) * K + k]);
    }

    const int nz = blockIdx.z;
    const int y = blockIdx.y;            // output row
    const int x0 = blockIdx.x * XO;      // output x base
    const int xvalid = min(2 * XO, W - 2 * x0);
    long long row_off[2] = {
        ((((long long)nz * H) + 2 * y) * W + 2 * x0) * C,
        ((((long long)nz * H) + 2 * y + 1) * W + 2 * x0) * C};
    stage_rows(s_in, in, row_off, 2, 2 * XO, xvalid, C, CPAD, tid, 256);
    __syncthreads();

    const long long out_row = (((long long)nz * HO) + y) * WO * K;

    for (int k = kslot; k < K; k += 32) {
        const float bj = bias ? bias[k] : 0.f;
        float acc[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) acc[p] = bj;
        for (int c = 0; c < C; ++c) {
            const float4 w4 =
                *reinterpret_cast<const float4*>(&s_w[(c * K + k) * 4]);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const int xl = 2 * (pslot + p * 8);  // local input x
                acc[p] += s_in[xl * CPAD + c] * w4.x;
                acc[p] += s_in[(xl + 1) * CPAD + c] * w4.y;
                acc[p] += s_in[(2 * XO + xl) * CPAD + c] * w4.z;
                acc[p] += s_in[(2 * XO + xl + 1) * CPAD + c] * w4.w;
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int xo = x0 + pslot + p * 8;
            if (xo >= WO) continue;
            stf(&out[out_row + (long long)xo * K + k], acc[p]);
        }
    }
}

// ---- input conv (1,5,5), pad (0,2,2), single input channel, on the MFMA --
// RSUNet's conv_in (1 -> 28). MIOpen's implicit GEMM collapses to a
// degenerate K-dim=25 GEMM here and runs ~39 ms (bf16) / ~7 ms (f32) per
// batch-24 launch. The VALU stencil this replaces (one thread per position,
// 25*K separate multiplies and adds under -ffp-contract=off, 7*K broadcast
// weight reads) took 1.02 ms for the 440 MB it writes at 12x20x256x256.
// out[n,z,y,x,k] = bias[k] + sum_t in[n,z,y+t/5-2,x+t%5-2] * w[k][t]
//
// As a GEMM: M = 16 consecutive x of one row (one tile), K = the 25 taps
// padded to 28 = 7 steps of v_mfma_f32_16x16x4_f32, N = K outputs padded
// to 32 = 2 column tiles; 14 MFMAs per tile. The accumulators start from
// the bias, so an output is the f32 fma chain over the taps in order.
//
// One workgroup = CI_R output rows x CI_S positions of one (n, z) plane:
// it stages (CI_R+4) x (CI_S+4) input values as f32 (zero outside the
// image in y and x -- a halo row is never a row of the neighbouring
// plane), 3.2 KB, loaded as one batch from clamped addresses and zeroed by
// a select after the load. Wave w then owns the 16-position column w of
// the strip and walks the rows with no further workgroup barrier.
// A: lane (i, kk) of step s reads the window value of tap t = 4s+kk for
// position i -- consecutive i are consecutive LDS words, one conflict-free
// ds_read_b32 per step; the padding taps t = 25..27 are selected to 0 (not
// multiplied by a zero weight: inf * 0 would poison the tile).
// B: 14 dwords per lane, gathered once per workgroup from wgt [K][25],
// zero for t >= 25 and for columns >= K.
// Epilogue: a tile's output is ONE contiguous run of 16*K elements, so the
// accumulators are bounced through a wave-private LDS copy of that run
// (D[row = position][col = k] -> s_b[position * K + k]; columns >= K are
// not written) and leave as 4-element pieces, piece f of the run at
// element 4f: 16-byte stores in f32, 8-byte in bf16. K % 4 != 0 or a
// misaligned `out` takes scalar stores; partial tiles select at the store.
// 11.2 KB of LDS, 62 VGPRs + 20 AGPRs: 5 workgroups, i.e. 5 waves per
// SIMD, per CU (6 in bf16), so one wave's bounce and stores hide under the
// MFMAs of the others. 12x20x256x256 f32: 0.405 ms for 1.82 GB of in +
// out, 4.5 TB/s (profiles/conv_in_mfma.json).
constexpr int CI_R = 8;             // output rows per workgroup
constexpr int CI_S = 64;            // output positions per workgroup
constexpr int CI_NW = CI_S / 16;    // waves, one 16-position column each
constexpr int CI_LW = CI_S + 4;     // staged row, floats

template <typename T>
__global__ __launch_bounds__(CI_NW * 64) void k_conv155_in_mfma(
    const T* __restrict__ in, const T* __restrict__ wgt,
    const float* __restrict__ bias, T* __restrict__ out, int H, int W,
    int K, int nstrips, int nrows, int vec_ok) {
    constexpr int NS = (CI_R + 4) * CI_LW;               // staged values
    constexpr int PER = (NS + CI_NW * 64 - 1) / (CI_NW * 64);
    __shared__ float s_in[NS];
    __shared__ __attribute__((aligned(16))) float s_bounce[CI_NW][16 * 32];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ai = lane & 15;   // A row (position) / B, D column
    const int akk = lane >> 4;  // A, B k / D row group
    // blockIdx.x = ((n*D + z) * nrows + row group) * nstrips + strip
    const int strip = (int)blockIdx.x % nstrips;
    const int rest = (int)blockIdx.x / nstrips;
    const int y0 = (rest % nrows) * CI_R;
    const int x0 = strip * CI_S;
    const long long plane = (long long)(rest / nrows) * H;

    // stage: every load first, from clamped addresses; zeros by select
    float v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int idx = u * (CI_NW * 64) + tid;
        const int r = idx / CI_LW;
        const int xl = idx - r * CI_LW;
        const int cy = min(max(y0 + r - 2, 0), H - 1);
        const int cx = min(max(x0 + xl - 2, 0), W - 1);
        v[u] = ldf(&in[(plane + cy) * W + cx]);
    }
    // B[k = akk][j = ai] of (step s, column tile t)
    float b[7][2];
#pragma unroll
    for (int s = 0; s < 7; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            b[s][t] = ldf(&wgt[min(16 * t + ai, K - 1) * 25 +
                               min(4 * s + akk, 24)]);
    float bj[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
        bj[t] = bias ? bias[min(16 * t + ai, K - 1)] : 0.f;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int idx = u * (CI_NW * 64) + tid;
        const int r = idx / CI_LW;
        const int xl = idx - r * CI_LW;
        const int gy = y0 + r - 2;
        const int gx = x0 + xl - 2;
        const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
        if (idx < NS) s_in[idx] = ok ? v[u] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 7; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            b[s][t] = 4 * s + akk < 25 && 16 * t + ai < K ? b[s][t] : 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) bj[t] = 16 * t + ai < K ? bj[t] : 0.f;
    __syncthreads();

    const int xt = x0 + 16 * wave;  // this wave's tile column
    if (xt >= W) return;
    const int nvalid = min(16, W - xt);
    const int rows = min(CI_R, H - y0);
    float* s_b = s_bounce[wave];
    // window offset of tap 4s + akk for position ai, row 0 of the strip
    int aoff[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int t = min(4 * s + akk, 24);
        aoff[s] = (t / 5) * CI_LW + (t % 5) + 16 * wave + ai;
    }
    const bool apad = 24 + akk >= 25;  // step 6 holds taps 24..27
    auto a_reads = [&](int ry, float (&a)[7]) {
#pragma unroll
        for (int s = 0; s < 7; ++s) a[s] = s_in[ry * CI_LW + aoff[s]];
        a[6] = apad ? 0.f : a[6];
    };

    float a[7];
    a_reads(0, a);
    for (int ry = 0; ry < rows; ++ry) {
        um_f32x4 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
            acc[t] = um_f32x4{bj[t], bj[t], bj[t], bj[t]};
#pragma unroll
        for (int s = 0; s < 7; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    a[s], b[s][t], acc[t], 0, 0, 0);
        // the next row's window, read while the MFMAs drain
        a_reads(min(ry + 1, rows - 1), a);
        // D[row = akk*4 + r][col = ai] -> the tile's output run
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (16 * t + ai < K) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s_b[(akk * 4 + r) * K + 16 * t + ai] = acc[t][r];
            }
        __builtin_amdgcn_wave_barrier();

        T* op = out + ((plane + y0 + ry) * W + xt) * (long long)K;
        if (vec_ok) {
            // every piece in registers first, then the stores back to back
            const int npiece = nvalid * (K >> 2);
            um_f32x4 p[2];
#pragma unroll
            for (int it = 0; it < 2; ++it)
                p[it] = *reinterpret_cast<const um_f32x4*>(
                    &s_b[4 * (it * 64 + lane)]);
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int f = it * 64 + lane;
                if (f >= npiece) continue;
                if (sizeof(T) == 2) {
                    typedef unsigned ci_u32x2
                        __attribute__((ext_vector_type(2)));
                    ci_u32x2 h;
                    h.x = bf16_bits(p[it][0]) |
                          ((unsigned)bf16_bits(p[it][1]) << 16);
                    h.y = bf16_bits(p[it][2]) |
                          ((unsigned)bf16_bits(p[it][3]) << 16);
                    reinterpret_cast<ci_u32x2*>(op)[f] = h;
                } else {
                    reinterpret_cast<um_f32x4*>(op)[f] = p[it];
                }
            }
        } else {
            const int ne = nvalid * K;
            for (int e = lane; e < ne; e += 64) stf(&op[e], s_b[e]);
        }
        __builtin_amdgcn_wave_barrier();  // the run is rewritten next row
    }
}

// ---- output conv (1,5,5), pad (0,2,2), 28 -> 3 channels, on the MFMA -----
// RSUNet's conv_out. N = 3 output channels would waste a 16-wide matrix
// tile, so the five x-taps are folded into the output dimension: for an
// output row y and staged positions x' the GEMM is
//   P[x'][j] = sum_{dy,c} in[y+dy-2][x'][c] * w[k][dy][dx][c],  j = dx*3+k
// (M = x', N = 15 real columns + one zero column, K = 5*28 = 140 = 35
// steps of v_mfma_f32_16x16x4_f32), and the output is the shifted sum
//   out[y][x][k] = bias[k] + sum_dx P[x+dx-2][dx*3+k].
//
// Fixed tiles; since k_conv155_out_ywalk below took the f32 route, this is
// the bf16 kernel (the f32 figures are kept as the record). One workgroup =
// CO_R = 6 output rows x CO_S = 60 output positions: it stages 10 input
// rows x 64 positions (x' = x0-2 .. x0+61, so both 2-column halos come
// from the workgroup's own strip) in the raw dtype, [row][x][c] with c
// stride 28. f32: 71,680 B of LDS -> 2 workgroups per CU (2 waves per
// SIMD); bf16: 35,840 B -> 4. Wave w owns the 16-position tile w for all
// 6 rows: an A fragment (lane (i, kk) reads in[row][16w+i][4s+kk]) is read
// once per staged row and feeds the up-to-5 output rows it is a dy tap
// of, i.e. 7 LDS reads per 35 MFMAs, and the 6 row accumulators are
// independent MFMA chains. The 35 B fragments (packed by the host as
// [dy*7+s][lane], lane = kk*16 + j) live in 35 VGPRs, loaded once.
// The shifted sum crosses lanes: P is bounced through LDS (over the
// input tile, [row][j][x'] with a 72-dword j stride so the b128 writes
// and reads spread over the banks); 90 threads then each produce 4
// consecutive positions x 3 channels = 12 contiguous outputs (3 x 16 B
// in f32, 3 x 8 B in bf16, when W % 4 == 0 and `out` is 16 B aligned;
// scalar stores otherwise).
// Cost of the fixed tiles: every staged row is read (6+4)/6 = 1.67x and
// every column 64/60 = 1.07x, 1.78x together (the repeats are L2 hits
// between neighbouring workgroups). x-waste at W = 256: 5 strips, the
// last holds 16 outputs and runs 2 of its 4 tiles, so 18 MFMA tiles for
// 16 tiles of output = 12.5 % over, on top of the 16/15 zero column.
// f32 accumulation, bf16 rounded once at the store.
constexpr int CO_R = 6;    // output rows per workgroup
constexpr int CO_S = 60;   // output positions per workgroup (64 staged)
constexpr int CO_PS = 72;  // P bounce: dwords between j rows

typedef float co_f32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(256, 2) void k_conv155_out_mfma(
    const T* __restrict__ in, const float* __restrict__ wfrag,
    const float* __restrict__ bias, T* __restrict__ out, int H, int W,
    int vec_ok) {
    constexpr int RS = CO_R + 4;           // staged rows
    constexpr int XS = 64;                 // staged positions
    constexpr int CC = 28, C4 = CC / 4;
    constexpr int NV = RS * XS * C4;       // 4-channel vectors to stage
    constexpr int PER = (NV + 255) / 256;  // per thread
    constexpr int BATCH = 6;               // loads in flight per thread
    static_assert(CO_R * 16 * CO_PS * 4 <= RS * XS * CC * (int)sizeof(T),
                  "P bounce must fit over the input tile");
    __shared__ __attribute__((aligned(16))) T s_in[RS * XS * CC];
    float* s_p = reinterpret_cast<float*>(s_in);  // after the MFMA phase

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int y0 = blockIdx.y * CO_R;
    const int x0 = blockIdx.x * CO_S;
    const long long plane = (long long)blockIdx.z * H;
    const int nout = min(CO_S, W - x0);      // valid outputs of this strip
    const int ntile = (nout + 4 + 15) >> 4;  // 16-position tiles needed

    float b[35];
#pragma unroll
    for (int s = 0; s < 35; ++s) b[s] = wfrag[s * 64 + lane];

    // stage: batched so the global loads pipeline; zero outside the image
    typedef typename vec4<T>::type tx4;
#pragma unroll 1
    for (int b0 = 0; b0 < PER; b0 += BATCH) {
        tx4 v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int idx = (b0 + u) * 256 + tid;
            const int r = idx / (XS * C4);
            const int rem = idx - r * (XS * C4);
            const int xl = rem / C4;
            const int c4 = rem - xl * C4;
            const int gy = y0 + r - 2;
            const int gx = x0 + xl - 2;
            const bool ok = b0 + u < PER && idx < NV && gy >= 0 &&
                            gy < H && gx >= 0 && gx < W &&
                            xl < ntile * 16;
            v[u] = ok ? *reinterpret_cast<const tx4*>(
                            &in[((plane + gy) * W + gx) * (long long)CC +
                                c4 * 4])
                      : tx4{};
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int idx = (b0 + u) * 256 + tid;
            if (b0 + u < PER && idx < NV)
                *reinterpret_cast<tx4*>(&s_in[idx * 4]) = v[u];
        }
    }
    __syncthreads();

    // MFMA phase: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15]
    co_f32x4 acc[CO_R];
#pragma unroll
    for (int y = 0; y < CO_R; ++y) acc[y] = co_f32x4{0.f, 0.f, 0.f, 0.f};
    if (wave < ntile) {
        const T* abase = &s_in[(wave * 16 + (lane & 15)) * CC + (lane >> 4)];
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            float a[C4];
#pragma unroll
            for (int s = 0; s < C4; ++s)
                a[s] = cvf(abase[r * XS * CC + s * 4]);
#pragma unroll
            for (int s = 0; s < C4; ++s)
#pragma unroll
                for (int dy = 0; dy < 5; ++dy) {
                    const int y = r - dy;  // staged row r is tap dy of y
                    if (y >= 0 && y < CO_R)
                        acc[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            a[s], b[dy * C4 + s], acc[y], 0, 0, 0);
                }
        }
    }
    __syncthreads();  // every A read done: the tile becomes the P bounce

    // D[row = (lane>>4)*4 + reg][col = lane&15] -> s_p[y][j][x']
    if (wave < ntile) {
#pragma unroll
        for (int y = 0; y < CO_R; ++y)
            *reinterpret_cast<co_f32x4*>(
                &s_p[(y * 16 + (lane & 15)) * CO_PS + wave * 16 +
                     (lane >> 4) * 4]) = acc[y];
    }
    __syncthreads();

    // shifted sum: thread = (row, 4 consecutive positions), 12 outputs
    if (tid >= CO_R * (CO_S / 4)) return;
    const int yl = tid / (CO_S / 4);
    const int q = tid - yl * (CO_S / 4);
    const int y = y0 + yl;
    const int gx = x0 + q * 4;
    if (y >= H || gx >= W) return;
    float o[4][3];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 3; ++k) o[e][k] = bias ? bias[k] : 0.f;
#pragma unroll
    for (int j = 0; j < 15; ++j) {
        const int dx = j / 3, k = j % 3;
        const float* pr = &s_p[(yl * 16 + j) * CO_PS + q * 4];
        const co_f32x4 lo = *reinterpret_cast<const co_f32x4*>(pr);
        const co_f32x4 hi = *reinterpret_cast<const co_f32x4*>(pr + 4);
        const float p8[8] = {lo[0], lo[1], lo[2], lo[3],
                             hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e][k] += p8[e + dx];
    }
    T* op = out + ((plane + y) * W + gx) * 3LL;
    if (vec_ok) {  // W % 4 == 0: the 4 positions exist and op is aligned
        if (sizeof(T) == 2) {
            typedef unsigned co_u32x2 __attribute__((ext_vector_type(2)));
            unsigned short h[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) h[i] = bf16_bits(o[i / 3][i % 3]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                co_u32x2 u;
                u.x = h[4 * i] | ((unsigned)h[4 * i + 1] << 16);
                u.y = h[4 * i + 2] | ((unsigned)h[4 * i + 3] << 16);
                reinterpret_cast<co_u32x2*>(op)[i] = u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                co_f32x4 f;
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    f[m] = o[(4 * i + m) / 3][(4 * i + m) % 3];
                reinterpret_cast<co_f32x4*>(op)[i] = f;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (gx + e < W)
#pragma unroll
                for (int k = 0; k < 3; ++k) stf(&op[e * 3 + k], o[e][k]);
    }
}

// ---- the same conv walking y: the f32 route ------------------------------
// Same GEMM, B fragments, accumulation order and shifted sum as
// k_conv155_out_mfma (the two are bit-equal), tiled the other way. A wave
// owns CY_XO = 12 output positions (16 staged, x' = xo-2 .. xo+13: tiles
// overlap by the 4-column halo, so a wave needs no neighbour and the
// kernel has no workgroup barrier) and a y segment of CY_YS rows of one
// (n, z) plane, and walks the input rows y0-2 .. y0+YS+1 in order. Input
// row r is tap dy of output row r-dy: five rolling accumulator chains are
// live, row r feeds all five (35 MFMAs on 7 A fragments), and output row
// r-4 is finished after it. The input is read (YS+4)/YS = 1.125x in y and
// 16/12 in x (neighbouring waves of a workgroup, L1/L2 hits) and nothing
// but one row tile is ever staged: 22 tiles per row at W = 256 against
// the fixed tiles' 18, 16/12 more MFMAs for no barrier.
// A row's 16 x 28 input values are one contiguous 1792-byte run: each
// lane loads two 16-byte pieces of it, a row ahead, and the run is staged
// in wave-private LDS, where lane (i, kk) reads in[x'+i][4s+kk] as
// s_a[i*28 + 4s + kk], conflict-free. (Taking the fragments straight from
// global, 7 dword loads per lane that each touch 16 separate 16-byte
// segments, was load-issue-bound: 1.36 ms against 1.05 ms this way and
// 1.26 ms for the fixed tiles, profiles/conv_in_mfma.json.)
// A finished row is bounced through wave-private LDS ([j][x'], 20-dword j
// stride); lanes 0..8 each sum 4 of the tile's 36 contiguous outputs, in
// the fixed-tile kernel's order, and store 16 bytes (one output per lane
// and scalar stores when W % 4 != 0 or `out` is misaligned). The stores
// are issued a row later, ahead of the next batch of loads, so the wait
// for those loads never waits for a young store (loads and stores share
// vmcnt). 113 VGPRs, 12 KB of LDS per workgroup: 4 waves per SIMD.
// f32 only: in bf16 the fixed tiles hold 4 workgroups per CU and stay
// faster (2.85 ms against 3.39 ms at 24x32x256x256).
constexpr int CY_YS = 32;   // output rows per wave
constexpr int CY_XO = 12;   // output positions per wave (16 staged)
constexpr int CY_NW = 4;    // waves per workgroup, independent
constexpr int CY_PS = 20;   // P bounce: dwords between j rows

__global__ __launch_bounds__(CY_NW * 64, 4) void k_conv155_out_ywalk(
    const float* __restrict__ in, const float* __restrict__ wfrag,
    const float* __restrict__ bias, float* __restrict__ out, int H, int W,
    int nxg, int nseg, int vec_ok) {
    constexpr int CC = 28, C4 = CC / 4;
    __shared__ __attribute__((aligned(16))) float s_bounce[CY_NW][16 * CY_PS];
    __shared__ __attribute__((aligned(16))) float s_tile[CY_NW][16 * CC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ai = lane & 15, akk = lane >> 4;
    const int xg = (int)blockIdx.x % nxg;
    const int rest = (int)blockIdx.x / nxg;
    const int y0 = (rest % nseg) * CY_YS;
    const long long plane = (long long)(rest / nseg) * H;
    const int xo = (xg * CY_NW + wave) * CY_XO;
    if (xo >= W) return;
    const int nout = min(CY_XO, W - xo);
    const int ys = min(CY_YS, H - y0);
    float* s_p = s_bounce[wave];
    float* s_a = s_tile[wave];

    float b[35];
#pragma unroll
    for (int s = 0; s < 35; ++s) b[s] = wfrag[s * 64 + lane];
    float bk[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) bk[k] = bias ? bias[k] : 0.f;

    // the tile's 16 x 28 input values of a row are one contiguous run of
    // 112 four-channel pieces: lane l loads pieces l and l + 64 (clamped:
    // lanes >= 48 repeat piece 111), coalesced, and the run is staged as it
    // is in wave-private LDS, where lane (i, kk) reads its A fragments
    // s_a[i*28 + 4s + kk] without bank conflicts
    unsigned poff[2];
    bool pok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int f = min(lane + 64 * j, 16 * C4 - 1);
        const int gx = xo - 2 + f / C4;
        pok[j] = gx >= 0 && gx < W;
        poff[j] = min(max(gx, 0), W - 1) * CC + 4 * (f % C4);
    }
    auto a_loads = [&](int r, co_f32x4 (&v)[2]) {
        const int cy = min(max(y0 - 2 + r, 0), H - 1);
        const float* ip = in + (plane + cy) * W * CC;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            v[j] = *reinterpret_cast<const co_f32x4*>(ip + poff[j]);
    };
    auto a_stage = [&](const co_f32x4 (&v)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            co_f32x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w[e] = pok[j] ? v[j][e] : 0.f;
            *reinterpret_cast<co_f32x4*>(
                &s_a[4 * min(lane + 64 * j, 16 * C4 - 1)]) = w;
        }
        __builtin_amdgcn_wave_barrier();
    };
    // P[x + dx][dx*3 + k] summed onto the bias, dx ascending
    auto outval = [&](int e) {
        const int x = e / 3, k = e - 3 * x;
        float o = k == 0 ? bk[0] : (k == 1 ? bk[1] : bk[2]);
#pragma unroll
        for (int dx = 0; dx < 5; ++dx)
            o += s_p[(dx * 3 + k) * CY_PS + x + dx];
        return o;
    };
    // a finished row: D[row = akk*4 + reg][col = ai] -> s_p[j][x'], then
    // this lane's outputs (4 consecutive of the 36, or one) in registers
    auto finish = [&](const co_f32x4& p) {
        *reinterpret_cast<co_f32x4*>(&s_p[ai * CY_PS + akk * 4]) = p;
        __builtin_amdgcn_wave_barrier();
        co_f32x4 o = co_f32x4{0.f, 0.f, 0.f, 0.f};
        if (vec_ok) {
            if (4 * lane < 3 * nout) {
#pragma unroll
                for (int m = 0; m < 4; ++m) o[m] = outval(4 * lane + m);
            }
        } else if (lane < 3 * nout) {
            o[0] = outval(lane);
        }
        __builtin_amdgcn_wave_barrier();  // s_p is rewritten next row
        return o;
    };
    // ... and its stores, issued a row later: ahead of the next batch of
    // loads, so that the wait for those loads never waits for a young store
    auto put = [&](int yl, const co_f32x4& o) {
        float* op = out + ((plane + y0 + yl) * W + xo) * 3LL;
        if (vec_ok) {
            if (4 * lane < 3 * nout)
                reinterpret_cast<co_f32x4*>(op)[lane] = o;
        } else if (lane < 3 * nout) {
            op[lane] = o[0];
        }
    };

    // acc[q] belongs to output row r - 4 + q while input row r is walked:
    // row r is tap dy of acc[4 - dy]
    co_f32x4 acc[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] = co_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nrow = ys + 4;  // input rows walked
    float a[C4];
    co_f32x4 an[2];
    co_f32x4 pend = co_f32x4{0.f, 0.f, 0.f, 0.f};
    a_loads(0, an);
    a_stage(an);
#pragma unroll 1
    for (int r = 0; r < nrow; ++r) {
        // the finished row's stores go out ahead of the next row's loads:
        // the wait for those loads (at a_stage, a row of MFMAs later) then
        // finds the store older still
        if (r >= 5) put(r - 5, pend);
        a_loads(min(r + 1, nrow - 1), an);
#pragma unroll
        for (int s = 0; s < C4; ++s) a[s] = s_a[ai * CC + 4 * s + akk];
        __builtin_amdgcn_wave_barrier();
        const int gy = y0 - 2 + r;
        if (r >= 4 && r < ys && gy < H) {  // all five taps live
#pragma unroll
            for (int s = 0; s < C4; ++s)
#pragma unroll
                for (int dy = 0; dy < 5; ++dy)
                    acc[4 - dy] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[s], b[dy * C4 + s], acc[4 - dy], 0, 0, 0);
        } else if (gy >= 0 && gy < H) {  // roll-in and roll-out
#pragma unroll
            for (int dy = 0; dy < 5; ++dy) {
                if (r - dy < 0 || r - dy >= ys) continue;
#pragma unroll
                for (int s = 0; s < C4; ++s)
                    acc[4 - dy] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[s], b[dy * C4 + s], acc[4 - dy], 0, 0, 0);
            }
        }
        if (r >= 4) pend = finish(acc[0]);  // output row r - 4 is done
        a_stage(an);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = acc[q + 1];
        acc[4] = co_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    put(ys - 1, pend);
}

// ---- one-pass epilogue for the convs left on MIOpen ----------------------
// y[v][k] = act(y[v][k] + bias[k] (+ res[v][k])), in place on an NDHWC f32
// tensor: the bias pass, the residual add and the ELU that torch runs as
// separate full-tensor kernels behind a MIOpen conv. ELU as in the ring
// epilogue: expm1f of the non-positive part, then a select (NaN stays NaN).
__device__ __forceinline__ float bre_act(float v, int do_elu) {
    if (do_elu) {
        const float e = expm1f(v > 0.f ? 0.f : v);
        v = v > 0.f ? v : e;
    }
    return v;
}

template <bool VEC>  // VEC: K % 4 == 0 and 16-byte aligned tensors
__global__ __launch_bounds__(256) void k_bias_res_elu(
    float* __restrict__ y, const float* __restrict__ bias,
    const float* __restrict__ res, long long total, int K, int do_elu) {
    const long long step = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const long long n4 = total >> 2;
        const int K4 = K >> 2;
        for (; i < n4; i += step) {
            const int k4 = (int)(i % K4);
            um_f32x4 v = reinterpret_cast<const um_f32x4*>(y)[i];
            if (bias) v += reinterpret_cast<const um_f32x4*>(bias)[k4];
            if (res) v += reinterpret_cast<const um_f32x4*>(res)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = bre_act(v[e], do_elu);
            reinterpret_cast<um_f32x4*>(y)[i] = v;
        }
    } else {
        for (; i < total; i += step) {
            float v = y[i];
            if (bias) v += bias[(int)(i % K)];
            if (res) v += res[i];
            y[i] = bre_act(v, do_elu);
        }
    }
}

}  // namespace

extern "C" int cfx_conv155_out(cfx_ctx* ctx, const void* in,
                               const float* wfrag, const float* bias,
                               void* out, int N, int D, int H, int W,
                               int C, int K, int is_bf16) {
    if (C != 28 || K != 3) {
        g_err = "cfx_conv155_out: only C == 28, K == 3 instantiated";
        return -1;
    }
    if ((long long)N * D > 65535) {
        g_err = "cfx_conv155_out: N * D <= 65535 supported";
        return -1;
    }
    if (!is_bf16 && (long long)N * D * ((H + CY_YS - 1) / CY_YS) *
                            ((W + CY_NW * CY_XO - 1) / (CY_NW * CY_XO)) >
                        0x7fffffffLL) {
        g_err = "cfx_conv155_out: too many workgroups for one grid axis";
        return -1;
    }
    dim3 grid((W + CO_S - 1) / CO_S, (H + CO_R - 1) / CO_R,
              (unsigned)(N * D));
    const int vec_ok = W % 4 == 0 && ((size_t)out & 15) == 0;
    double flops = 2.0 * 25.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV_STREAM, flops, [&] {
        if (is_bf16) {
            // bf16 stays on the fixed tiles: 4 workgroups per CU there, and
            // the y-walk measured slower (profiles/conv_in_mfma.json)
            hipLaunchKernelGGL((k_conv155_out_mfma<cfx_bf16>), grid,
                               dim3(256), 0, ctx->stream,
                               (const cfx_bf16*)in, wfrag, bias,
                               (cfx_bf16*)out, H, W, vec_ok);
        } else {
            const int nxg = (W + CY_NW * CY_XO - 1) / (CY_NW * CY_XO);
            const int nseg = (H + CY_YS - 1) / CY_YS;
            const long long nwg = (long long)N * D * nseg * nxg;
            if (nwg > 0)
                hipLaunchKernelGGL(k_conv155_out_ywalk, dim3((unsigned)nwg),
                                   dim3(CY_NW * 64), 0, ctx->stream,
                                   (const float*)in, wfrag, bias,
                                   (float*)out, H, W, nxg, nseg, vec_ok);
        }
        return 0;
    });
}

extern "C" int cfx_conv155_c1(cfx_ctx* ctx, const void* in, const void* wgt,
                              const float* bias, void* out, int N, int D,
                              int H, int W, int K, int is_bf16) {
    if (K > 32) {
        g_err = "cfx_conv155_c1: K <= 32 supported";
        return -1;
    }
    if (K < 1 || N < 0 || D < 0 || H < 1 || W < 1) {
        g_err = "cfx_conv155_c1: K >= 1, N, D >= 0, H, W >= 1";
        return -1;
    }
    // one flat grid axis over (plane, row group, strip): no 65535 limit
    const int nstrips = (W + CI_S - 1) / CI_S;
    const int nrows = (H + CI_R - 1) / CI_R;
    const long long nwg = (long long)N * D * nrows * nstrips;
    if (nwg > 0x7fffffffLL) {
        g_err = "cfx_conv155_c1: N * D * ceil(H/8) * ceil(W/64) < 2^31 "
                "supported";
        return -1;
    }
    if (nwg == 0) return 0;
    const int vec_ok = K % 4 == 0 && ((size_t)out & 15) == 0;
    double flops = 2.0 * 25.0 * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV_STREAM, flops, [&] {
        if (is_bf16)
            hipLaunchKernelGGL((k_conv155_in_mfma<cfx_bf16>),
                               dim3((unsigned)nwg), dim3(CI_NW * 64), 0,
                               ctx->stream, (const cfx_bf16*)in,
                               (const cfx_bf16*)wgt, bias, (cfx_bf16*)out, H,
                               W, K, nstrips, nrows, vec_ok);
        else
            hipLaunchKernelGGL((k_conv155_in_mfma<float>),
                               dim3((unsigned)nwg), dim3(CI_NW * 64), 0,
                               ctx->stream, (const float*)in,
                               (const float*)wgt, bias, (float*)out, H, W, K,
                               nstrips, nrows, vec_ok);
        return 0;
    });
}

namespace {

// LDS of k_upconv2_mfma: the B fragments + one bounce per wave
size_t um_shmem(int C, int K) {
    return ((size_t)C * 4 * K + (size_t)UM_NW * 16 * (4 * K + 4)) *
           sizeof(float);
}

// shapes the MFMA up-conv takes: whole MFMA steps and 16-byte channel
// runs, 16-byte aligned tensors, a tile count that fits an int; K <= 48
// (NT <= 12, RSUNet's widest up-conv) is instantiated -- there the
// accumulators, the skip batch and the two A sets already take 195 VGPRs
// + 144 AGPRs, one wave per SIMD
bool um_eligible(const void* in, const void* skip, const void* out, int N,
                 int D, int H, int W, int C, int K) {
    return C % 4 == 0 && K % 4 == 0 && C >= 4 && C <= 64 && K >= 4 &&
           K <= 48 && (((size_t)in | (size_t)skip | (size_t)out) & 15) == 0 &&
           (long long)N * D * H * ((W + 15) / 16) < (1LL << 31);
}

template <int NT, bool SKIP>
int um_launch_nt(cfx_ctx* ctx, const float* in, const float* wgt,
                 const float* bias, const float* skip, float* out, int W,
                 int C, int xtiles, int ntiles) {
    const size_t shmem = um_shmem(C, 4 * NT);
    if (shmem > 64 * 1024)
        CFX_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_upconv2_mfma<NT, SKIP>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    int cus = 0;
    CFX_CHECK(hipDeviceGetAttribute(
        &cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    // persistent: as many workgroups as the LDS lets a CU hold
    const int per_cu = (int)std::min<size_t>(8, (160 * 1024) / shmem);
    const int grid =
        std::min((ntiles + UM_NW - 1) / UM_NW, std::max(1, cus * per_cu));
    hipLaunchKernelGGL((k_upconv2_mfma<NT, SKIP>), dim3(grid),
                       dim3(UM_NW * 64), shmem, ctx->stream, in, wgt, bias,
                       skip, out, W, C, xtiles, ntiles);
    return 0;
}

template <bool SKIP>
int um_launch(cfx_ctx* ctx, const float* in, const float* wgt,
              const float* bias, const float* skip, float* out, int N,
              int D, int H, int W, int C, int K) {
    const int xtiles = (W + 15) / 16;
    const int ntiles = N * D * H * xtiles;
    if (ntiles == 0) return 0;
    switch (K / 4) {
#define UM_CASE(NT)                                                         \
    case NT:                                                                \
        return um_launch_nt<NT, SKIP>(ctx, in, wgt, bias, skip, out, W, C,  \
                                      xtiles, ntiles);
        UM_CASE(1) UM_CASE(2) UM_CASE(3) UM_CASE(4) UM_CASE(5) UM_CASE(6)
        UM_CASE(7) UM_CASE(8) UM_CASE(9) UM_CASE(10) UM_CASE(11)
        UM_CASE(12)
#undef UM_CASE
    }
    g_err = "upconv mfma: K not instantiated";
    return -1;
}

// the timed MFMA up-conv, with (SKIP) or without the skip-add epilogue;
// zero tiles launch nothing and still push their row
template <bool SKIP>
int um_timed(cfx_ctx* ctx, const void* in, const void* wgt,
             const float* bias, const void* skip, void* out, int N, int D,
             int H, int W, int C, int K) {
    double flops = 2.0 * 4.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV_STREAM, flops, [&] {
        return um_launch<SKIP>(ctx, (const float*)in, (const float*)wgt,
                               bias, (const float*)skip, (float*)out, N, D,
                               H, W, C, K);
    });
}

}  // namespace

extern "C" int cfx_upconv_2x2_add(cfx_ctx* ctx, const void* in,
                                  const void* wgt, const float* bias,
                                  const void* skip, void* out, int N, int D,
                                  int H, int W, int C, int K, int is_bf16) {
    if (!skip)
        return cfx_upconv_2x2(ctx, in, wgt, bias, out, N, D, H, W, C, K,
                              is_bf16);
    if (is_bf16) {
        g_err = "cfx_upconv_2x2_add: skip is f32 only";
        return -1;
    }
    if (!um_eligible(in, skip, out, N, D, H, W, C, K)) {
        g_err = "cfx_upconv_2x2_add: skip needs C % 4 == 0, K % 4 == 0, "
                "C <= 64, K <= 48 and 16-byte aligned tensors";
        return -1;
    }
    return um_timed<true>(ctx, in, wgt, bias, skip, out, N, D, H, W, C, K);
}

extern "C" int cfx_upconv_2x2(cfx_ctx* ctx, const void* in, const void* wgt,
                              const float* bias, void* out, int N, int D,
                              int H, int W, int C, int K, int is_bf16) {
    if (K > 64 || C > 64) {
        g_err = "cfx_upconv_2x2: C, K <= 64 supported";
        return -1;
    }
    if (!is_bf16 && um_eligible(in, nullptr, out, N, D, H, W, C, K))
        return um_timed<false>(ctx, in, wgt, bias, nullptr, out, N, D, H, W,
                               C, K);
    constexpr int XI = 64;
    dim3 grid((W + XI - 1) / XI, H, (unsigned)(N * D));
    const size_t shmem =
        ((size_t)C * K * 4 + (size_t)XI * (C | 1)) * sizeof(float);
    double flops = 2.0 * 4.0 * C * K * (double)N * D * H * W;
    return cfx_timed(ctx, CFX_K_CONV_STREAM, flops, [&] {
        if (is_bf16)
            hipLaunchKernelGGL((k_upconv2<cfx_bf16, XI>), grid, dim3(256),
                               shmem, ctx->stream, (const cfx_bf16*)in,
                               (const cfx_bf16*)wgt, bias, (cfx_bf16*)out, N,
                               D, H, W, C, K);
        else
            hipLaunchKernelGGL((k_upconv2<float, XI>), grid, dim3(256),
                               shmem, ctx->stream, (const float*)in,
                               (const float*)wgt, bias, (float*)out, N, D, H,
                               W, C, K);
        return 0;
    });
}

extern "C" int cfx_downconv_2x2(cfx_ctx* ctx, const void* in,
                                const void* wgt, const float* bias,
                                void* out, int N, int D, int H, int W,
                                int C, int K, int is_bf16) {
    if (K > 64 || C > 64) {
        g_err = "cfx_downconv_2x2: C, K <= 64 supported";
        return -1;
    }
    if ((H | W) & 1) {
        g_err = "cfx_downconv_2x2: H, W must be even";
        return -1;
    }
    constexpr int XO = 64;
    dim3 grid((W / 2 + XO - 1) / XO, H / 2, (unsigned)(N * D));
    const size_t shmem =
        ((size_t)C * K * 4 + (size_t)2 * 2 * XO * (C | 1)) * sizeof(float);
    double flops = 2.0 * 4.0 * C * K * (double)N * D * (H / 2) * (W / 2);
    return cfx_timed(ctx, CFX_K_CONV_STREAM, flops, [&] {
        if (is_bf16)
            hipLaunchKernelGGL((k_downconv2<cfx_bf16, XO>), grid, dim3(256),
                               shmem, ctx->stream, (const cfx_bf16*)in,
                               (const cfx_bf16*)wgt, bias, (cfx_bf16*)out, N,
                               D, H, W, C, K);
        else
            hipLaunchKernelGGL((k_downconv2<float, XO>), grid, dim3(256),
                               shmem, ctx->stream, (const float*)in,
                               (const float*)wgt, bias, (float*)out, N, D, H,
                               W, C, K);
        return 0;
    });
}

extern "C" int cfx_bias_res_elu(cfx_ctx* ctx, float* y, const float* bias,
                                const float* res, long long nvox, int K,
                                int do_elu) {
    if (nvox < 0 || K < 1) {
        g_err = "cfx_bias_res_elu: nvox >= 0, K >= 1";
        return -1;
    }
    const long long total = nvox * K;
    if (total == 0) return 0;
    const bool vec =
        K % 4 == 0 &&
        (((size_t)y | (size_t)bias | (size_t)res) & 15) == 0;
    const long long items = vec ? total / 4 : total;
    // a few resident workgroups per CU, grid-stride
    const int grid = (int)std::min<long long>((items + 255) / 256, 256 * 16);
    if (vec)
        hipLaunchKernelGGL((k_bias_res_elu<true>), dim3(grid), dim3(256), 0,
                           ctx->stream, y, bias, res, total, K, do_elu);
    else
        hipLaunchKernelGGL((k_bias_res_elu<false>), dim3(grid), dim3(256), 0,
                           ctx->stream, y, bias, res, total, K, do_elu);
    CFX_CHECK(hipGetLastError());
    return 0;
}
