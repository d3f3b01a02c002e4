// Shared host/device helpers for liblime_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/lime_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void lime_set_error(const char* fmt, ...);
void lime_set_last_linear_kernel(const char* fmt, ...);      // lime_last_linear_kernel(): which instantiation ran

#define LIME_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            lime_set_error(__VA_ARGS__);         \
            return (code);                       \
        }                                        \
    } while (0)

// compute units of the current device: queried once, 256 when there is no device to ask (common.cpp)
int lime_num_cus();

// 16-byte vector access to rows of `ld` floats from `ptr` is possible (a NULL operand is absent, hence fine)
static inline bool lime_al16(const void* ptr, long ld) { return ptr == nullptr || (((uintptr_t)ptr % 16) == 0 && (ld % 4) == 0); }

// called right after a kernel launch; never synchronises
static inline int lime_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lime_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return LIME_ERR_LAUNCH;
    }
    return LIME_OK;
}

// Raise `kernel`'s dynamic-LDS limit to `bytes`, once: `reserved` is the caller's static (one per kernel instantiation, 0 at first)
// and keeps the largest size granted, so a launch that fits makes no runtime call.  `entry`: the entry point the message names.
static inline int lime_reserve_lds(const void* kernel, int bytes, int& reserved, const char* entry) {
    if (bytes <= reserved) return LIME_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    LIME_REQUIRE(e == hipSuccess, LIME_ERR_LAUNCH, "%s: cannot reserve %d bytes of LDS: %s", entry, bytes, hipGetErrorString(e));
    reserved = bytes;
    return LIME_OK;
}

// workgroups of a persistent kernel that walks `ntiles` tiles: `per_cu` per compute unit, one per tile at the most
static inline long lime_persistent_grid(long ntiles, int per_cu = 1) {
    const long nwg = (long)lime_num_cus() * per_cu;
    return nwg < ntiles ? nwg : ntiles;
}

// workgroups of a grid-stride kernel: one per `per` of the `total` items, `cap` at the most
static inline unsigned lime_grid_cap(long total, int per, int cap) {
    const long g = (total + per - 1) / per;
    return (unsigned)(g > cap ? cap : g);
}

__device__ __forceinline__ float wave_half_sum(float v) {
    // sum over the 32 lanes of this lane's half-wave (xor offsets < 32 never cross the halves)
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}
__device__ __forceinline__ float wave_half_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, __shfl_xor(v, 4));
    v = fmaxf(v, __shfl_xor(v, 2));
    v = fmaxf(v, __shfl_xor(v, 1));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    v = wave_half_sum(v);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    v = wave_half_max(v);
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

// A round's pick of the greedy selections over a shortlist (mmr_rows_f32.hip, calibrate_rows.hip): the better of two (v, rank) is the
// larger v, the lower rank on equal v ("no entry": v = -inf, rank = INT_MAX); wave_best_pick leaves the wave's best in every lane.
struct best_pick {
    float v;
    int j;
};
__device__ __forceinline__ best_pick better_pick(best_pick a, best_pick b) { return (b.v > a.v || (b.v == a.v && b.j < a.j)) ? b : a; }
__device__ __forceinline__ best_pick wave_best_pick(best_pick a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = better_pick(a, best_pick{__shfl_xor(a.v, m), __shfl_xor(a.j, m)});
    return a;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a workgroup-scope fence + s_barrier, and the fence
// also waits vmcnt(0): every global load still in flight (a prefetch) and every store (an epilogue) would be drained
// at each barrier.  The kernels here exchange data between waves through LDS only.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// The same for ONE wave.  LDS ops of a wave execute in order; drain lgkmcnt so that a tile written by some lanes is read back by
// others, and keep the compiler from moving memory ops across the point.  Deliberately NOT a workgroup-scope fence: that also
// waits vmcnt(0), i.e. for the prefetches and the output stores still in flight.
__device__ __forceinline__ void wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Sum / maximum over the 256 threads (four waves) of a workgroup, in a fixed order; `red` is >= 4 floats of LDS; every thread gets
// the result.  The barrier in front of the write protects `red` against the readers of its previous use: safe back to back.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// The first two thirds of a softmax over the LDS array a[0 .. n), by the 256 threads of a workgroup: a[i] <- exp(a[i] - max a),
// returns 1 / sum of them (the caller scales where it uses the terms).  Thread t touches the elements t, t + 256, ... only: values it
// wrote itself need no barrier in front, and the caller puts one behind before other threads read `a`.
__device__ __forceinline__ float block_softmax_terms(float* a, int n, float* red) {
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, a[i]);
    mx = block_max(mx, red);
    float part = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float e = expf(a[i] - mx);
        a[i] = e;
        part += e;
    }
    return 1.0f / block_sum(part, red);
}

__device__ __forceinline__ float lime_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the run-time activation of the lime_linear_f32 epilogues (LIME_ACT_RELU_GRAD is a backward pass of its own, not an activation)
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == LIME_ACT_RELU) return fmaxf(v, 0.f);
    if (act == LIME_ACT_TANH) return tanhf(v);
    if (act == LIME_ACT_SIGMOID) return lime_sigmoid(v);
    return v;
}

// Four consecutive elements 4 j .. 4 j + 3 of a row of n floats (zeros behind the end; VEC: one 16-byte load), and the dot product /
// axpy over such a quad with explicit fmaf in element order: the kernels whose bits must not depend on their form use these.
// (J: the caller's index width, int or long.)
template <bool VEC, typename J>
__device__ __forceinline__ f32x4 row_quad(const float* __restrict__ p, J j, int n) {
    const J e = 4 * j;
    if (VEC) return *reinterpret_cast<const f32x4*>(p + e);
    f32x4 r;
    r.x = e < n ? p[e] : 0.f;
    r.y = e + 1 < n ? p[e + 1] : 0.f;
    r.z = e + 2 < n ? p[e + 2] : 0.f;
    r.w = e + 3 < n ? p[e + 3] : 0.f;
    return r;
}
__device__ __forceinline__ float fma_dot4(f32x4 a, f32x4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ f32x4 fma_axpy4(float a, f32x4 x, f32x4 acc) {
    acc.x = fmaf(a, x.x, acc.x);
    acc.y = fmaf(a, x.y, acc.y);
    acc.z = fmaf(a, x.z, acc.z);
    acc.w = fmaf(a, x.w, acc.w);
    return acc;
}

// The remaining-lifetime weight (util.py:23-49), the expression of lime_interest_match_f32 / lime_lifetime_score_f32:
// positive_mask * w + negative_mask * beta * w with the expired penalty, sigmoid(alpha |r|) without
__device__ __forceinline__ float lifetime_weight(float r, float alpha_s, float beta_s, int use_penalty) {
    float w;
    if (use_penalty) {
        w = lime_sigmoid(alpha_s * r);
        w = (r >= 0.f ? 1.f : 0.f) * w + (r < 0.f ? 1.f : 0.f) * beta_s * w;
    } else {
        w = lime_sigmoid(alpha_s * fabsf(r));
    }
    return w;
}

// XCD-aware bijective remap of a 1-D grid: the 8 XCDs take workgroups round-robin by blockIdx, so
// logical ids are handed out such that each XCD walks one contiguous range (tiles that share
// operand panels then share an L2).  Placement only changes speed, never results.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}
