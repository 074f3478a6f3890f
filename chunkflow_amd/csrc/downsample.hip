// Downsample kernels: box averaging (uint8 / float32 images and affinity
// maps) and COUNTLESS mode pooling (32/64-bit label volumes). Semantics are
// pinned bit-exactly to the numpy implementation the reference ships
// (lib/igneous/downsample.py, called as downsample_upload.py:67-75 does);
// the rules are spelled out in chunkflow_amd/downsample.py.
//
// All of these are bandwidth-bound: N bytes in, N/4 or N/8 out. Layout is
// contiguous (C,) z-y-x with x fastest. Each entry point has
//   * a general kernel: one lane per output voxel, any shape / factor;
//   * a vector kernel for 16-byte-aligned rows: one lane loads 16 contiguous
//     bytes from every input row of its cell group (consecutive lanes take
//     consecutive 16-byte chunks of the same rows, 1 KiB per wave per load)
//     and writes 8 or 16 contiguous output bytes.
// Rows whose pitch or base is not 16-byte aligned take the general kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "cfx_internal.h"

namespace {

constexpr int kBlock = 256;

inline int grid_for(long long items) {
    long long want = (items + kBlock - 1) / kBlock;
    return (int)std::min<long long>(std::max<long long>(want, 1), 1 << 20);
}

inline bool aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <typename T, int N>
union Vec {
    uint4 q;
    uint2 h;
    T e[N];
};

// ---------------------------------------------------------------------------
// averaging: f32 sum (x-offset slowest, z-offset fastest), f64 quotient,
// then round-to-nearest (f32) or truncate (u8)
// ---------------------------------------------------------------------------
template <typename T>
__device__ inline T avg_finish(float sum, int count) {
    return (T)((double)sum / (double)count);
}

template <typename T>
__global__ void k_avg_general(const T* __restrict__ in, T* __restrict__ out,
                              long long n_out, int D, int H, int W, int oD,
                              int oH, int oW, int fz, int fy, int fx) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_out; idx += stride) {
        int ox = (int)(idx % oW);
        long long t = idx / oW;
        int oy = (int)(t % oH);
        t /= oH;
        int oz = (int)(t % oD);
        long long c = t / oD;
        int z0 = oz * fz, y0 = oy * fy, x0 = ox * fx;
        int nz = min(fz, D - z0), ny = min(fy, H - y0), nx = min(fx, W - x0);
        const T* base = in + ((c * D + z0) * H + y0) * (long long)W + x0;
        float sum = 0.0f;
        for (int dx = 0; dx < nx; ++dx)
            for (int dy = 0; dy < ny; ++dy)
                for (int dz = 0; dz < nz; ++dz)
                    sum += (float)base[((long long)dz * H + dy) * W + dx];
        out[idx] = avg_finish<T>(sum, nz * ny * nx);
    }
}

// factors in {1,2}; W * sizeof(T) a multiple of 16 (so W % FX == 0 too)
template <typename T, int FX>
__global__ void k_avg_vec(const T* __restrict__ in, T* __restrict__ out,
                          long long n_items, int D, int H, int W, int oD,
                          int oH, int fz, int fy) {
    constexpr int E = 16 / (int)sizeof(T);  // inputs per lane per row
    constexpr int NO = E / FX;              // outputs per lane
    const int chunks = W / E;
    const int oW = W / FX;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_items; idx += stride) {
        int xi = (int)(idx % chunks);
        long long t = idx / chunks;
        int oy = (int)(t % oH);
        t /= oH;
        int oz = (int)(t % oD);
        long long c = t / oD;
        int z0 = oz * fz, y0 = oy * fy;
        int nz = min(fz, D - z0), ny = min(fy, H - y0);
        Vec<T, E> v[2][2];
#pragma unroll
        for (int dz = 0; dz < 2; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
                if (dz < nz && dy < ny)
                    v[dz][dy].q = *reinterpret_cast<const uint4*>(
                        in + ((c * D + z0 + dz) * H + y0 + dy) * (long long)W
                        + (long long)xi * E);
        // count is 1, 2, 4 or 8 here, so sum / count is an exact power-of-
        // two scaling: the f64 quotient is exact and its conversion to T
        // (one rounding for f32, truncation for u8) equals that of the f32
        // product below, without f64 division on the streaming path
        const float inv = 1.0f / (float)(nz * ny * FX);
        Vec<T, E> o;
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            float sum = 0.0f;
#pragma unroll
            for (int dx = 0; dx < FX; ++dx)
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dz = 0; dz < 2; ++dz)
                        if (dz < nz && dy < ny)
                            sum += (float)v[dz][dy].e[j * FX + dx];
            o.e[j] = (T)(sum * inv);
        }
        T* dst = out + ((c * oD + oz) * oH + oy) * (long long)oW
                 + (long long)xi * NO;
        if (FX == 1)
            *reinterpret_cast<uint4*>(dst) = o.q;
        else
            *reinterpret_cast<uint2*>(dst) = o.h;
    }
}

// The same lane layout for uint8, in packed integer arithmetic: a sum of at
// most eight uint8 values is an exact integer in f32, f64 and here alike, and
// truncating its exact quotient by 2^shift is a right shift. Each 32-bit
// word is split into its even and odd bytes (two 16-bit fields per word, max
// field value 8 * 255), which keeps the byte unpacking off the VALU's
// convert path and the register count low.
template <int FX>
__global__ void k_avg_vec_u8(const unsigned char* __restrict__ in,
                             unsigned char* __restrict__ out,
                             long long n_items, int D, int H, int W, int oD,
                             int oH, int fz, int fy) {
    constexpr unsigned int M = 0x00ff00ffu;
    const int chunks = W / 16;
    const int oW = W / FX;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_items; idx += stride) {
        int xi = (int)(idx % chunks);
        long long t = idx / chunks;
        int oy = (int)(t % oH);
        t /= oH;
        int oz = (int)(t % oD);
        long long c = t / oD;
        int z0 = oz * fz, y0 = oy * fy;
        int nz = min(fz, D - z0), ny = min(fy, H - y0);
        Vec<unsigned int, 4> v[2][2];
#pragma unroll
        for (int dz = 0; dz < 2; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
                if (dz < nz && dy < ny)
                    v[dz][dy].q = *reinterpret_cast<const uint4*>(
                        in + ((c * D + z0 + dz) * H + y0 + dy) * (long long)W
                        + (long long)xi * 16);
        const int shift = (nz == 2) + (ny == 2) + (FX == 2);
        unsigned int even[4], odd[4];  // per word: bytes 0,2 and bytes 1,3
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned int se = 0, so = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
                    if (dz < nz && dy < ny) {
                        se += v[dz][dy].e[w] & M;
                        so += (v[dz][dy].e[w] >> 8) & M;
                    }
            even[w] = se;
            odd[w] = so;
        }
        unsigned char* dst = out + ((c * oD + oz) * oH + oy) * (long long)oW
                             + (long long)xi * (16 / FX);
        if (FX == 1) {
            Vec<unsigned int, 4> o;
#pragma unroll
            for (int w = 0; w < 4; ++w)
                o.e[w] = ((even[w] >> shift) & M)
                         | (((odd[w] >> shift) & M) << 8);
            *reinterpret_cast<uint4*>(dst) = o.q;
        } else {
            unsigned int r[4];  // outputs 2w and 2w+1 at bits 0..7, 16..23
#pragma unroll
            for (int w = 0; w < 4; ++w)
                r[w] = ((even[w] + odd[w]) >> shift) & M;
            uint2 o;
            o.x = ((r[0] | (r[0] >> 8)) & 0xffffu)
                  | ((r[1] | (r[1] >> 8)) << 16);
            o.y = ((r[2] | (r[2] >> 8)) & 0xffffu)
                  | ((r[3] | (r[3] >> 8)) << 16);
            *reinterpret_cast<uint2*>(dst) = o;
        }
    }
}

template <typename T, int FX>
void launch_avg_vec(cfx_ctx* ctx, const T* in, T* out, long long items,
                    int D, int H, int W, int oD, int oH, int fz, int fy) {
    if constexpr (std::is_same<T, unsigned char>::value)
        hipLaunchKernelGGL(k_avg_vec_u8<FX>, dim3(grid_for(items)),
                           dim3(kBlock), 0, ctx->stream, in, out, items, D,
                           H, W, oD, oH, fz, fy);
    else
        hipLaunchKernelGGL((k_avg_vec<T, FX>), dim3(grid_for(items)),
                           dim3(kBlock), 0, ctx->stream, in, out, items, D,
                           H, W, oD, oH, fz, fy);
}

template <typename T>
int launch_avg(cfx_ctx* ctx, const T* in, T* out, int channels,
               const int in_dims[3], const int factor[3]) {
    int D = in_dims[0], H = in_dims[1], W = in_dims[2];
    int fz = factor[0], fy = factor[1], fx = factor[2];
    if (channels <= 0 || D <= 0 || H <= 0 || W <= 0) {
        g_err = "downsample_avg: empty input";
        return -1;
    }
    if (fz <= 0 || fy <= 0 || fx <= 0) {
        g_err = "downsample_avg: factors must be positive";
        return -1;
    }
    int oD = (D + fz - 1) / fz, oH = (H + fy - 1) / fy,
        oW = (W + fx - 1) / fx;
    bool vec = fz <= 2 && fy <= 2 && fx <= 2 &&
               ((long long)W * sizeof(T)) % 16 == 0 && aligned16(in) &&
               aligned16(out);
    if (vec) {
        long long items =
            (long long)channels * oD * oH * (W / (16 / (int)sizeof(T)));
        if (fx == 2)
            launch_avg_vec<T, 2>(ctx, in, out, items, D, H, W, oD, oH, fz,
                                 fy);
        else
            launch_avg_vec<T, 1>(ctx, in, out, items, D, H, W, oD, oH, fz,
                                 fy);
    } else {
        long long n_out = (long long)channels * oD * oH * oW;
        hipLaunchKernelGGL(k_avg_general<T>, dim3(grid_for(n_out)),
                           dim3(kBlock), 0, ctx->stream, in, out, n_out, D,
                           H, W, oD, oH, oW, fz, fy, fx);
    }
    CFX_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// COUNTLESS 2D: per slice of the preserved axis, a if a==b or a==c, else b
// if b==c, else d. An odd pooled axis is front-mirrored ([v0,v0,v1,..]):
// padded index j reads source max(j - odd, 0).
// ---------------------------------------------------------------------------
template <typename T>
__host__ __device__ inline T pick2d(T a, T b, T c, T d) {
    return (a == b || a == c) ? a : (b == c ? b : d);
}

__device__ inline int src_lo(int o, int odd) { return max(2 * o - odd, 0); }
__device__ inline int src_hi(int o, int odd) { return 2 * o + 1 - odd; }

template <typename T>
__global__ void k_mode2_general(const T* __restrict__ in,
                                T* __restrict__ out, long long n_out, int D,
                                int H, int W, int oD, int oH, int oW, int p) {
    long long stride = (long long)gridDim.x * blockDim.x;
    const int first = (p == 0) ? 1 : 0;  // first pooled axis
    const int dims[3] = {D, H, W};
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_out; idx += stride) {
        int o[3];
        o[2] = (int)(idx % oW);
        long long t = idx / oW;
        o[1] = (int)(t % oH);
        o[0] = (int)(t / oH);
        int lo[3], hi[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            int odd = dims[ax] & 1;
            lo[ax] = (ax == p) ? o[ax] : src_lo(o[ax], odd);
            hi[ax] = (ax == p) ? o[ax] : src_hi(o[ax], odd);
        }
        int bi[3], ci[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            bi[ax] = (ax == first) ? lo[ax] : hi[ax];
            ci[ax] = (ax == first) ? hi[ax] : lo[ax];
        }
        auto at = [&](const int* i) {
            return in[((long long)i[0] * H + i[1]) * W + i[2]];
        };
        out[idx] = pick2d<T>(at(lo), at(bi), at(ci), at(hi));
    }
}

// x pooled (p = 0 or 1), W * sizeof(T) a multiple of 16 (so W is even): two
// input rows (lo / hi of the other pooled axis) of 16 bytes -> 8 bytes out
template <typename T>
__global__ void k_mode2_vec_xpool(const T* __restrict__ in,
                                  T* __restrict__ out, long long n_items,
                                  int D, int H, int W, int oD, int oH,
                                  int p) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int NO = E / 2;
    const int chunks = W / E;
    const int oW = W / 2;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_items; idx += stride) {
        int xi = (int)(idx % chunks);
        long long t = idx / chunks;
        int oy = (int)(t % oH);
        int oz = (int)(t / oH);
        int z0, z1, y0, y1;
        if (p == 0) {
            z0 = z1 = oz;
            y0 = src_lo(oy, H & 1);
            y1 = src_hi(oy, H & 1);
        } else {
            y0 = y1 = oy;
            z0 = src_lo(oz, D & 1);
            z1 = src_hi(oz, D & 1);
        }
        Vec<T, E> r0, r1, o;
        r0.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z0 * H + y0) * W + (long long)xi * E);
        r1.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z1 * H + y1) * W + (long long)xi * E);
#pragma unroll
        for (int j = 0; j < NO; ++j)
            o.e[j] = pick2d<T>(r0.e[2 * j], r0.e[2 * j + 1], r1.e[2 * j],
                               r1.e[2 * j + 1]);
        *reinterpret_cast<uint2*>(out + ((long long)oz * oH + oy) * oW
                                  + (long long)xi * NO) = o.h;
    }
}

// x preserved (p = 2), W * sizeof(T) a multiple of 16: four input rows of
// 16 bytes -> 16 bytes out
template <typename T>
__global__ void k_mode2_vec_xkeep(const T* __restrict__ in,
                                  T* __restrict__ out, long long n_items,
                                  int D, int H, int W, int oD, int oH) {
    constexpr int E = 16 / (int)sizeof(T);
    const int chunks = W / E;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_items; idx += stride) {
        int xi = (int)(idx % chunks);
        long long t = idx / chunks;
        int oy = (int)(t % oH);
        int oz = (int)(t / oH);
        int z0 = src_lo(oz, D & 1), z1 = src_hi(oz, D & 1);
        int y0 = src_lo(oy, H & 1), y1 = src_hi(oy, H & 1);
        long long x = (long long)xi * E;
        Vec<T, E> a, b, c, d, o;
        a.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z0 * H + y0) * W + x);
        b.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z0 * H + y1) * W + x);
        c.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z1 * H + y0) * W + x);
        d.q = *reinterpret_cast<const uint4*>(
            in + ((long long)z1 * H + y1) * W + x);
#pragma unroll
        for (int j = 0; j < E; ++j)
            o.e[j] = pick2d<T>(a.e[j], b.e[j], c.e[j], d.e[j]);
        *reinterpret_cast<uint4*>(out + ((long long)oz * oH + oy) * W + x) =
            o.q;
    }
}

template <typename T>
int launch_mode2(cfx_ctx* ctx, const T* in, T* out, const int in_dims[3],
                 int p) {
    int D = in_dims[0], H = in_dims[1], W = in_dims[2];
    int oD = (p == 0) ? D : (D + 1) / 2;
    int oH = (p == 1) ? H : (H + 1) / 2;
    int oW = (p == 2) ? W : (W + 1) / 2;
    constexpr int E = 16 / (int)sizeof(T);
    bool vec = ((long long)W * sizeof(T)) % 16 == 0 && aligned16(in) &&
               aligned16(out);
    if (vec) {
        long long items = (long long)oD * oH * (W / E);
        if (p == 2)
            hipLaunchKernelGGL(k_mode2_vec_xkeep<T>, dim3(grid_for(items)),
                               dim3(kBlock), 0, ctx->stream, in, out, items,
                               D, H, W, oD, oH);
        else
            hipLaunchKernelGGL(k_mode2_vec_xpool<T>, dim3(grid_for(items)),
                               dim3(kBlock), 0, ctx->stream, in, out, items,
                               D, H, W, oD, oH, p);
    } else {
        long long n_out = (long long)oD * oH * oW;
        hipLaunchKernelGGL(k_mode2_general<T>, dim3(grid_for(n_out)),
                           dim3(kBlock), 0, ctx->stream, in, out, n_out, D,
                           H, W, oD, oH, oW, p);
    }
    CFX_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// COUNTLESS 3D over the eight voxels s = 4*dx + 2*dy + dz of a 2x2x2 block:
// value of the lexicographically first all-equal 4-combination, else of the
// first 3-combination, else of the first equal pair among s = 0..6, else
// voxel 7. Equal-value classes are disjoint, so the lexicographically first
// k-combination belongs to the class (of size >= k) whose lowest index is
// smallest: count matches per voxel and keep the lowest qualifying index.
// ---------------------------------------------------------------------------
template <typename T>
__host__ __device__ inline T pick3d(const T (&v)[8]) {
    int cnt[8];  // matches over all eight, self included
#pragma unroll
    for (int i = 0; i < 8; ++i) cnt[i] = 1;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i + 1; j < 8; ++j) {
            int eq = (v[i] == v[j]) ? 1 : 0;
            cnt[i] += eq;
            cnt[j] += eq;
        }
    T r = v[7];
#pragma unroll
    for (int i = 6; i >= 0; --i)  // matches over s = 0..6 only
        if (cnt[i] - ((v[i] == v[7]) ? 1 : 0) >= 2) r = v[i];
#pragma unroll
    for (int i = 7; i >= 0; --i)
        if (cnt[i] >= 3) r = v[i];
#pragma unroll
    for (int i = 7; i >= 0; --i)
        if (cnt[i] >= 4) r = v[i];
    return r;
}

template <typename T>
__global__ void k_mode3_general(const T* __restrict__ in,
                                T* __restrict__ out, long long n_out, int H,
                                int W, int oH, int oW) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_out; idx += stride) {
        int ox = (int)(idx % oW);
        long long t = idx / oW;
        int oy = (int)(t % oH);
        long long oz = t / oH;
        const T* base = in + ((2 * oz) * H + 2 * oy) * (long long)W + 2 * ox;
        T v[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            int dx = s >> 2, dy = (s >> 1) & 1, dz = s & 1;
            v[s] = base[((long long)dz * H + dy) * W + dx];
        }
        out[idx] = pick3d<T>(v);
    }
}

// W * sizeof(T) a multiple of 16: four input rows of 16 bytes -> 8 bytes out
template <typename T>
__global__ void k_mode3_vec(const T* __restrict__ in, T* __restrict__ out,
                            long long n_items, int H, int W, int oH) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int NO = E / 2;
    const int chunks = W / E;
    const int oW = W / 2;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < n_items; idx += stride) {
        int xi = (int)(idx % chunks);
        long long t = idx / chunks;
        int oy = (int)(t % oH);
        long long oz = t / oH;
        const T* base =
            in + ((2 * oz) * H + 2 * oy) * (long long)W + (long long)xi * E;
        Vec<T, E> r[2][2];  // [dz][dy]
#pragma unroll
        for (int dz = 0; dz < 2; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
                r[dz][dy].q = *reinterpret_cast<const uint4*>(
                    base + ((long long)dz * H + dy) * W);
        Vec<T, E> o;
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            T v[8];
#pragma unroll
            for (int s = 0; s < 8; ++s)
                v[s] = r[s & 1][(s >> 1) & 1].e[2 * j + (s >> 2)];
            o.e[j] = pick3d<T>(v);
        }
        *reinterpret_cast<uint2*>(out + (oz * oH + oy) * (long long)oW
                                  + (long long)xi * NO) = o.h;
    }
}

template <typename T>
int launch_mode3(cfx_ctx* ctx, const T* in, T* out, const int in_dims[3]) {
    int D = in_dims[0], H = in_dims[1], W = in_dims[2];
    int oD = D / 2, oH = H / 2, oW = W / 2;
    constexpr int E = 16 / (int)sizeof(T);
    bool vec = ((long long)W * sizeof(T)) % 16 == 0 && aligned16(in) &&
               aligned16(out);
    if (vec) {
        long long items = (long long)oD * oH * (W / E);
        hipLaunchKernelGGL(k_mode3_vec<T>, dim3(grid_for(items)),
                           dim3(kBlock), 0, ctx->stream, in, out, items, H,
                           W, oH);
    } else {
        long long n_out = (long long)oD * oH * oW;
        hipLaunchKernelGGL(k_mode3_general<T>, dim3(grid_for(n_out)),
                           dim3(kBlock), 0, ctx->stream, in, out, n_out, H,
                           W, oH, oW);
    }
    CFX_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int cfx_downsample_avg_u8(cfx_ctx* ctx, const unsigned char* in,
                                     unsigned char* out, int channels,
                                     const int in_dims[3],
                                     const int factor[3]) {
    return launch_avg<unsigned char>(ctx, in, out, channels, in_dims, factor);
}

extern "C" int cfx_downsample_avg_f32(cfx_ctx* ctx, const float* in,
                                      float* out, int channels,
                                      const int in_dims[3],
                                      const int factor[3]) {
    return launch_avg<float>(ctx, in, out, channels, in_dims, factor);
}

extern "C" int cfx_downsample_mode2(cfx_ctx* ctx, const void* in, void* out,
                                    int elem_bytes, const int in_dims[3],
                                    int preserved_axis) {
    if (in_dims[0] <= 0 || in_dims[1] <= 0 || in_dims[2] <= 0) {
        g_err = "downsample_mode2: empty input";
        return -1;
    }
    if (preserved_axis < 0 || preserved_axis > 2) {
        g_err = "downsample_mode2: preserved_axis must be 0, 1 or 2";
        return -1;
    }
    if (elem_bytes == 4)
        return launch_mode2<unsigned int>(
            ctx, static_cast<const unsigned int*>(in),
            static_cast<unsigned int*>(out), in_dims, preserved_axis);
    if (elem_bytes == 8)
        return launch_mode2<unsigned long long>(
            ctx, static_cast<const unsigned long long*>(in),
            static_cast<unsigned long long*>(out), in_dims, preserved_axis);
    g_err = "downsample_mode2: elem_bytes must be 4 or 8";
    return -1;
}

extern "C" int cfx_downsample_mode3(cfx_ctx* ctx, const void* in, void* out,
                                    int elem_bytes, const int in_dims[3]) {
    if (in_dims[0] <= 0 || in_dims[1] <= 0 || in_dims[2] <= 0) {
        g_err = "downsample_mode3: empty input";
        return -1;
    }
    if ((in_dims[0] | in_dims[1] | in_dims[2]) & 1) {
        g_err = "downsample_mode3: every dimension must be even";
        return -1;
    }
    if (elem_bytes == 4)
        return launch_mode3<unsigned int>(
            ctx, static_cast<const unsigned int*>(in),
            static_cast<unsigned int*>(out), in_dims);
    if (elem_bytes == 8)
        return launch_mode3<unsigned long long>(
            ctx, static_cast<const unsigned long long*>(in),
            static_cast<unsigned long long*>(out), in_dims);
    g_err = "downsample_mode3: elem_bytes must be 4 or 8";
    return -1;
}
