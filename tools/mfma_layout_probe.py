"""Empirically verify the v_mfma_f32_32x32x16_bf16 fragment layout.

Hypothesis (CDNA pattern): A[i][k]: lane l holds i = l&31, k = 8*(l>>5)+e
for e = 0..7 (bf16 pairs k=2j,2j+1 per VGPR); B[k][j]: j = l&31,
k = 8*(l>>5)+e; D (f32x16): col j = l&31, row = (reg&3) + 8*(reg>>2) +
4*(l>>5). Asymmetric A and B catch any transpose (guide G9).
"""
import os
import subprocess
import sys

import numpy as np

SRC = r'''
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

extern "C" __global__ void probe16(const bf16* A /*16x32 row-major*/,
                                   const bf16* B /*32x16 row-major*/,
                                   float* D /*16x16 row-major*/) {
    int l = threadIdx.x;
    bf16x8 a, b;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    for (int e = 0; e < 8; ++e) {
        int k = 8 * (l >> 4) + e;
        a[e] = A[(l & 15) * 32 + k];      // A[i][k]
        b[e] = B[k * 16 + (l & 15)];      // B[k][j]
    }
    f32x4 acc = {};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) {
        int row = (l >> 4) * 4 + r;       // C/D: col=lane&15, row=(l>>4)*4+r
        D[row * 16 + (l & 15)] = acc[r];
    }
}

extern "C" __global__ void probe(const bf16* A /*32x16 row-major*/,
                                 const bf16* B /*16x32 row-major*/,
                                 float* D /*32x32 row-major*/) {
    int l = threadIdx.x;
    bf16x8 a, b;
    for (int e = 0; e < 8; ++e) {
        int k = 8 * (l >> 5) + e;
        a[e] = A[(l & 31) * 16 + k];      // A[i][k]
        b[e] = B[k * 32 + (l & 31)];      // B[k][j]
    }
    f32x16 acc = {};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 16; ++r) {
        int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        D[row * 32 + (l & 31)] = acc[r];
    }
}
'''


def main():
    import torch
    here = '/tmp/mfma_probe'
    os.makedirs(here, exist_ok=True)
    import ctypes
    rng = np.random.RandomState(0)
    A = (rng.randn(32, 16) * 0.5).astype(np.float32)
    B = (rng.randn(16, 32) * 0.5).astype(np.float32)
    tA = torch.from_numpy(A).to(torch.bfloat16).cuda()
    tB = torch.from_numpy(B).to(torch.bfloat16).cuda()
    tD = torch.zeros(32, 32, dtype=torch.float32, device='cuda')

    with open(f'{here}/launch.hip', 'w') as f:
        f.write(SRC + r'''
extern "C" int run(const void* a, const void* b, void* d) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0,
                       (const bf16*)a, (const bf16*)b, (float*)d);
    return (int)hipDeviceSynchronize();
}
extern "C" int run16(const void* a, const void* b, void* d) {
    hipLaunchKernelGGL(probe16, dim3(1), dim3(64), 0, 0,
                       (const bf16*)a, (const bf16*)b, (float*)d);
    return (int)hipDeviceSynchronize();
}
''')
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O2', '-fPIC',
                    '-shared', f'{here}/launch.hip', '-o',
                    f'{here}/launch.so'], check=True)
    lib = ctypes.CDLL(f'{here}/launch.so')
    rc = lib.run(ctypes.c_void_p(tA.data_ptr()),
                 ctypes.c_void_p(tB.data_ptr()),
                 ctypes.c_void_p(tD.data_ptr()))
    print('rc', rc)
    got = tD.cpu().numpy()
    ref = (tA.float().cpu().numpy() @ tB.float().cpu().numpy())
    err = np.abs(got - ref).max()
    print('max err vs bf16-rounded ref:', err)
    print('match:', err < 0.05)
    if err >= 0.05:
        # localize: check a few entries
        print('got[0,:4]', got[0, :4], 'ref[0,:4]', ref[0, :4])
        print('got[:4,0]', got[:4, 0], 'ref[:4,0]', ref[:4, 0])

    # 16x16x32 variant
    A2 = (rng.randn(16, 32) * 0.5).astype(np.float32)
    B2 = (rng.randn(32, 16) * 0.5).astype(np.float32)
    tA2 = torch.from_numpy(A2).to(torch.bfloat16).cuda()
    tB2 = torch.from_numpy(B2).to(torch.bfloat16).cuda()
    tD2 = torch.zeros(16, 16, dtype=torch.float32, device='cuda')
    rc = lib.run16(ctypes.c_void_p(tA2.data_ptr()),
                   ctypes.c_void_p(tB2.data_ptr()),
                   ctypes.c_void_p(tD2.data_ptr()))
    got2 = tD2.cpu().numpy()
    ref2 = (tA2.float().cpu().numpy() @ tB2.float().cpu().numpy())
    err2 = np.abs(got2 - ref2).max()
    print('16x16x32 rc', rc, 'max err:', err2, 'match:', err2 < 0.05)
    if err2 >= 0.05:
        print('got2[0,:4]', got2[0, :4], 'ref2[0,:4]', ref2[0, :4])
        print('got2[:4,0]', got2[:4, 0], 'ref2[:4,0]', ref2[:4, 0])


# ---- f32 multi-block MFMA: v_mfma_f32_4x4x1_16b_f32 ----------------------
# `--f32-blocks [OUT.json]`: (1) fragment layout with cbsz = abid = blgp = 0
# against the hypothesis A[block = l>>2][i = l&3], B[block][j = l&3],
# D register i at lane 4*block + j (asymmetric random A and B); (2) issue
# cost beside v_mfma_f32_16x16x4_f32: one wave per SIMD, operands in
# registers, s_memtime around 10^4 iterations of 4 steps, one step being
# 1 x 16x16x4 (+ N4 x 4x4x1 on their own accumulators). SPLIT alternates
# the 16-wide accumulator between two chains (the ring's kk-parity split).
SRC_F32_BLOCKS = r'''
#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void layout4(const float* A /*16x4*/, const float* B /*16x4*/,
                        float* D /*16x4x4: [block][i][j]*/) {
    const int l = threadIdx.x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(A[(l >> 2) * 4 + (l & 3)],
                                             B[(l >> 2) * 4 + (l & 3)],
                                             acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i)
        D[((l >> 2) * 4 + i) * 4 + (l & 3)] = acc[i];
}

template <int N4, int SPLIT>
__global__ void issue_cost(float* sink, long long* cyc, int iters) {
    const int l = threadIdx.x & 63;
    const float a = 1e-3f * (float)(l + 1);
    const float b = 1e-3f * (float)(64 - l);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = acc;
    f32x4 c4[3] = {acc, acc, acc};
    __builtin_amdgcn_sched_barrier(0);
    const long long t0 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4& d = (SPLIT && (u & 1)) ? acc2 : acc;
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0);
#pragma unroll
            for (int t = 0; t < N4; ++t)
                c4[t] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c4[t], 0,
                                                           0, 0);
            __builtin_amdgcn_sched_barrier(0);  // keep the steps apart
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const long long t1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    float s = 0.f;
    for (int r = 0; r < 4; ++r)
        s += acc[r] + acc2[r] + c4[0][r] + c4[1][r] + c4[2][r];
    sink[threadIdx.x] = s;
    if (l == 0) cyc[threadIdx.x >> 6] = t1 - t0;
}

#define CK(x) do { if ((x) != hipSuccess) return -1; } while (0)

extern "C" int run_layout4(const float* A, const float* B, float* D) {
    float *dA, *dB, *dD;
    CK(hipMalloc(&dA, 256)); CK(hipMalloc(&dB, 256));
    CK(hipMalloc(&dD, 1024));
    CK(hipMemcpy(dA, A, 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B, 256, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(layout4, dim3(1), dim3(64), 0, 0, dA, dB, dD);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D, dD, 1024, hipMemcpyDeviceToHost));
    hipFree(dA); hipFree(dB); hipFree(dD);
    return 0;
}

// one workgroup of 4 waves = one wave per SIMD of one CU
extern "C" int run_issue_cost(int variant, int iters, long long* cyc4) {
    float* sink; long long* cyc;
    CK(hipMalloc(&sink, 256 * 4)); CK(hipMalloc(&cyc, 4 * 8));
    for (int rep = 0; rep < 2; ++rep) {  // first launch warms up
        switch (variant) {
        case 0: hipLaunchKernelGGL((issue_cost<0, 1>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        case 1: hipLaunchKernelGGL((issue_cost<1, 1>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        case 2: hipLaunchKernelGGL((issue_cost<3, 1>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        case 3: hipLaunchKernelGGL((issue_cost<0, 0>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        case 4: hipLaunchKernelGGL((issue_cost<1, 0>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        case 5: hipLaunchKernelGGL((issue_cost<3, 0>), dim3(1), dim3(256),
                                   0, 0, sink, cyc, iters); break;
        default: return -2;
        }
        CK(hipDeviceSynchronize());
    }
    CK(hipMemcpy(cyc4, cyc, 32, hipMemcpyDeviceToHost));
    hipFree(sink); hipFree(cyc);
    return 0;
}
'''


def main_f32_blocks(out_path=None):
    import ctypes
    import json
    import tempfile
    here = tempfile.mkdtemp(prefix='mfma_f32_blocks_')
    with open(f'{here}/probe.hip', 'w') as f:
        f.write(SRC_F32_BLOCKS)
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-fPIC',
                    '-shared', f'{here}/probe.hip', '-o',
                    f'{here}/probe.so'], check=True)
    lib = ctypes.CDLL(f'{here}/probe.so')
    fp = ctypes.POINTER(ctypes.c_float)

    rng = np.random.RandomState(0)
    A = rng.randn(16, 4).astype(np.float32)
    B = (rng.randn(16, 4) * 3 + 1).astype(np.float32)
    D = np.full((16, 4, 4), np.nan, np.float32)
    rc = lib.run_layout4(A.ctypes.data_as(fp), B.ctypes.data_as(fp),
                         D.ctypes.data_as(fp))
    assert rc == 0, rc
    ref = A[:, :, None] * B[:, None, :]           # [block][i][j], exact f32
    match = bool(np.array_equal(D, ref))
    print('4x4x1_16b layout A[l>>2][l&3] B[l>>2][l&3] D reg i @ lane '
          '4*block+j  match:', match)
    if not match:
        print('got[0]', D[0], 'ref[0]', ref[0], sep='\n')

    iters = 10000
    names = ['16x16x4 (2 chains)', '16x16x4 (2 chains) + 1 x 4x4x1',
             '16x16x4 (2 chains) + 3 x 4x4x1', '16x16x4 (1 chain)',
             '16x16x4 (1 chain) + 1 x 4x4x1',
             '16x16x4 (1 chain) + 3 x 4x4x1']
    cost = {}
    for v, name in enumerate(names):
        cyc = (ctypes.c_longlong * 4)()
        rc = lib.run_issue_cost(v, iters, cyc)
        assert rc == 0, rc
        per = sorted(c / (iters * 4.0) for c in cyc)
        cost[name] = round((per[1] + per[2]) / 2, 2)  # median of 4 waves
        print(f'{name}: {cost[name]} cyc/step  (waves {per})')
    base = cost[names[0]]
    t4_1 = cost[names[1]] - base
    t4_3 = (cost[names[2]] - base) / 3
    result = {
        'instruction': 'v_mfma_f32_4x4x1_16b_f32',
        'layout_hypothesis': 'A[block=l>>2][i=l&3] B[block][j=l&3] '
                             'D reg i at lane 4*block+j',
        'layout_match': match,
        'iters': iters, 'steps_per_iter': 4,
        'cycles_per_step': cost,
        't4_from_1': round(t4_1, 2), 't4_from_3': round(t4_3, 2),
    }
    print(json.dumps(result))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump({'mfma_probe': result}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    if '--f32-blocks' in sys.argv:
        i = sys.argv.index('--f32-blocks')
        main_f32_blocks(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
    else:
        main()
