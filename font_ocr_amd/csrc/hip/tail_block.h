// tail_block.h — "the kernel's last workgroup does the prefix": the device helpers the tail's kernels share (rows.hip, verify.hip,
// order.hip).  A header, not a .hip: there is no relocatable device code, so a kernel and the device functions it calls share a
// translation unit.
#pragma once
#include "common.h"

namespace focr {

// exclusive prefix of n u32 counts by ONE workgroup: base[0..n] (base[n] = total); *total_out = total, *max_out = max
// (u64 each; either may be null); zero[0..n) is cleared on the way if given (the scatter's per-row cursors).  Each of the 16
// waves owns a contiguous segment (a multiple of 256 entries) and walks it 256 entries at a time — 16-byte loads, coalesced
// — twice: sums first, then the prefix.  The arrays are padded to a multiple of 4 entries by their owner (rows2_begin).
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
// the prefix as the work of ONE 1 024-thread workgroup: a kernel of its own (row_prefix_kernel, rows.hip), or the last workgroup of the
// kernel that produced the counts (the hits-first tail's verify: a launch less in the batch's chain of kernels)
__device__ __forceinline__ void row_prefix_block(const uint32_t *__restrict__ cnt, uint32_t n, uint32_t *__restrict__ base, uint32_t *__restrict__ zero,
                                                 uint64_t *__restrict__ total_out, uint64_t *__restrict__ max_out, uint32_t *wave_sum, uint32_t *wave_max) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t seg = ((n + 15) / 16 + 255) / 256 * 256, b = min(n, wv * seg), e = min(n, b + seg);
    const v4u *cnt4 = reinterpret_cast<const v4u *>(cnt);
    uint32_t sum = 0, mx = 0;
    for (uint32_t i0 = b + 4 * lane; i0 < e; i0 += 4 * 256) {
        v4u vv[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            vv[q] = v4u{0, 0, 0, 0};
            if (i0 + q * 256 < e) vv[q] = cnt4[(i0 + q * 256) / 4];  // entries past n (inside the padding) are zero
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            sum += vv[q][0] + vv[q][1] + vv[q][2] + vv[q][3];
            mx = max(max(mx, max(vv[q][0], vv[q][1])), max(vv[q][2], vv[q][3]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += (uint32_t)__shfl_xor((int)sum, o);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    }
    if (lane == 0) {
        wave_sum[wv] = sum;
        wave_max[wv] = mx;
    }
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t q = 0; q < wv; q++) carry += wave_sum[q];
    for (uint32_t i00 = b; i00 < e; i00 += 4 * 256) {  // four tiles' loads in flight, then their scans
        v4u vv[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = i00 + q * 256 + 4 * lane;
            vv[q] = v4u{0, 0, 0, 0};
            if (i < e) vv[q] = cnt4[i / 4];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = i00 + q * 256 + 4 * lane;
            const v4u v = vv[q];
            const uint32_t tot4 = v[0] + v[1] + v[2] + v[3];
            uint32_t incl = tot4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(incl, o);
                if ((int)lane >= o) incl += u;
            }
            if (i < e) {
                const uint32_t p0 = carry + incl - tot4;
                reinterpret_cast<v4u *>(base)[i / 4] = v4u{p0, p0 + v[0], p0 + v[0] + v[1], p0 + v[0] + v[1] + v[2]};
                if (zero) reinterpret_cast<v4u *>(zero)[i / 4] = v4u{0, 0, 0, 0};
            }
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();  // base[n] below may share a 16-byte group with the last wave's stores
    if (threadIdx.x == 0) {
        uint32_t tot = 0, m = 0;
        for (int q = 0; q < 16; q++) {
            tot += wave_sum[q];
            m = max(m, wave_max[q]);
        }
        base[n] = tot;
        if (total_out) *total_out = tot;
        if (max_out) *max_out = m;
    }
}

// "Am I the kernel's last workgroup?" — called by every thread of a workgroup when its work is done.  The last one to arrive sees
// everything the others wrote (their release at the counter, its acquire here: the L1 of this CU may hold lines another CU has
// rewritten since) and may go on with work that needs all of it: the launch it saves stood 40-50 us in a batch's chain of kernels
// whenever other batches' kernels filled the chip.
struct TailWork {
    uint32_t *done;  // zeroed with the scan's counters (ClearList)
    uint32_t n_rows;
    uint32_t *hbase;
    uint64_t *total_out, *max_out;
};
__device__ __forceinline__ bool last_workgroup(uint32_t *done) {
    __shared__ uint32_t is_last;
    __syncthreads();  // the workgroup's stores have left its waves (workgroup-scope release: they are in this XCD's L2) ...
    if (threadIdx.x == 0) {
        // ... and ONE agent-scope release writes that L2's dirty lines back for the other XCDs (a workgroup lives on one XCD).  Not one
        // per thread: 8 192 L2 write-backs per launch instead of 512 doubled the verify's time alone on the chip (183 -> 383 us).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        is_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (is_last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (threadIdx.x == 0) *done = 0;  // zero between launches (and zeroed with the scan's counters anyway)
    }
    return is_last != 0;
}

}  // namespace focr
