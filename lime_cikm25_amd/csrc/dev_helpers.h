// The device helpers every kernel file shares, defined ONCE (tests/test_kernel_resources.py keeps the .hip files from growing copies):
// buffer resources and buffer loads / stores, LDS-DMA, counted vmcnt waits, the XOR swizzle of the [row][64-byte] LDS image, bf16
// packing, AccVGPR reads, the 16-lane row sum, the recomputed lane id.  Everything is __forceinline__; gfx950 only.
// (common.h: the fp32 vector types, wave reductions, lds_barrier, xcd_remap and the host helpers.  split_mfma.h: the split product.)
#pragma once
#include "common.h"

// Diagnostic builds only (-DLIME_STAMPS, tools/*_stamps.py): add the s_memtime since the last stamp to segment i of the kernel's local
// tsum[] / tlast.  Empty in liblime_hip.so.
#ifdef LIME_STAMPS
#define LIME_STAMP(i)                                                       \
    {                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                  \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();         \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                 \
        tsum[i] += t_ - tlast;                                              \
        tlast = t_;                                                         \
        __builtin_amdgcn_sched_barrier(0);                                  \
    }
#else
#define LIME_STAMP(i)
#endif

namespace lime_dev {

constexpr unsigned OOB = 0x80000000u;              // a buffer offset beyond num_records: loads / DMAs return zeros, stores are dropped
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFF0, 0x00020000);
}
// 16 bytes per lane global -> LDS (lane l lands at lds_base + 16 l); out-of-range offsets write zeros.  Counts in vmcnt.
// (The builtin only exists in the device pass; inside a kernel TEMPLATE it makes the host pass drop the launch stub.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, void* lds_base, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)lds_base, 16, voff, soff, 0, 0);
#endif
}
// "all but the N youngest vector-memory operations of this wave are done" (loads, stores and LDS-DMA count together, in
// issue order: MI355X_MICROARCH.md)
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// Workgroup barrier with LDS-DMA left in flight across it (never __syncthreads(): its fence drains vmcnt)
__device__ __forceinline__ void ring_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Bit 31 of a buffer offset (beyond num_records: zeros come back, nothing is read or written) when one of `a`, `b` is negative.  The
// branch-free form of `cond ? offset : OOB`: written as a select, hipcc turns a test shared by a group of loads into divergent control
// flow -- two exec-masked loads into the same registers with a `s_waitcnt vmcnt(0)` between them, and a join that waits in front of
// the MFMAs.
__device__ __forceinline__ unsigned dead_bit(int a, int b) { return (unsigned)(a | b) & OOB; }
// vmcnt(0), and the registers the wave's loads land in pass through the statement: hipcc's own bookkeeping does not see a wait in
// inline asm and would put `s_waitcnt vmcnt(..)` of its own in front of the registers' first use, behind younger loads and DMAs.
// (One statement for all of them: in front of a statement of its own each register gets hipcc's counted wait again.)
__device__ __forceinline__ void wait_vm0_landed(f32x4& a, f32x4& b) {
    wait_vm<0>();
    asm volatile("" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void wait_vm0_landed(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    wait_vm<0>();
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

// A device-side count (the compacted rows / sequences of this launch, written by an earlier kernel of the stream) against the host's
// bound `cap`: `cap` when there is none, else the count clamped to 0 .. cap, wave-uniform.
__device__ __forceinline__ int live_count(const int* dev, int cap) {
    if (dev) {
        const int m = __builtin_amdgcn_readfirstlane(*dev);
        cap = m < cap ? (m > 0 ? m : 0) : cap;
    }
    return cap;
}

// The lane id, recomputed where it is called (the opaque zero keeps hipcc from hoisting it -- and everything derived from it -- out
// of the tile loop, where the values would sit in registers through every step or be spilled: scratch reloads wait vmcnt(0)).
__device__ __forceinline__ int lane_here() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}

// One accumulator register -> a VGPR, HERE.  Left to itself hipcc copies every accumulator of a kernel out of the AccVGPRs in front
// of the first VALU use (160 copies ahead of a store epilogue: the VGPR file overflows and loop-carried values go to scratch);
// the "a" constraint keeps the value in its AccVGPR until this instruction.  The caller puts mfma_settle() between the last MFMA
// and the first of these: inline asm is outside the compiler's MFMA hazard bookkeeping.
__device__ __forceinline__ float acc_read(float a) {
    float v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}
__device__ __forceinline__ f32x4 acc_read4(const f32x4& a) { return f32x4{acc_read(a[0]), acc_read(a[1]), acc_read(a[2]), acc_read(a[3])}; }
__device__ __forceinline__ void mfma_settle() {        // > the 16 cycles of a v_mfma_f32_16x16x32_bf16 plus its write-back
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    // v_mfma_f32_16x16x4_f32: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; c[r] = C[4 (l >> 4) + r][l & 15]
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The attention kernels take their scores to the log2 domain: p = exp2(s' - max') is one v_exp_f32
constexpr float LOG2E = 1.4426950408889634f;

// Swizzle of the [row][four 16-byte segments] LDS image: physical segment = logical ^ swz4((row >> 2) & 3).  ds_read_b128 is serviced
// in four NON-contiguous 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, +32 for the other two; MI355X_MICROARCH.md, LDS):
// with the MFMA 16x16 lane layout (row = lane & 15, k slot = lane >> 4) a group mixes rows 0-3 / 12-15 of one k slot with rows 4-11 of
// another, and the plain XOR with (r >> 2) & 3 put two rows of every group on each 16-byte slot (SQ_LDS_BANK_CONFLICT = 49 % of the
// LDS cycles).  The permutation {0, 2, 3, 1} of (r >> 2) & 3 makes all four groups conflict free.
__device__ __forceinline__ int swz4(int q) { return (0x78 >> (2 * q)) & 3; }

// two floats -> two bf16 in one register, round to nearest even: ONE v_cvt_pk_bf16_f32 on gfx950 (the integer form -- add 0x7FFF +
// lsb, shift, merge -- is nine VALU instructions per pair: 4.6k of a wave's 5.8k VALU instructions per tile in the feed-forward kernel)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
}
__device__ __forceinline__ f32x4 unpack_bf16x4(u32x2 v) {
    f32x4 r;
    r[0] = __builtin_bit_cast(float, v[0] << 16);
    r[1] = __builtin_bit_cast(float, v[0] & 0xFFFF0000u);
    r[2] = __builtin_bit_cast(float, v[1] << 16);
    r[3] = __builtin_bit_cast(float, v[1] & 0xFFFF0000u);
    return r;
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 buf_load4_bf16(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {     // 4 bf16 -> 4 floats
    return unpack_bf16x4(__builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0)));
}
__device__ __forceinline__ int buf_load_i32(__amdgpu_buffer_rsrc_t r, unsigned voff) {
    return (int)__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0);
}
__device__ __forceinline__ void buf_store4(f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_store4_bf16(f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    u32x2 o;
    o[0] = pack_bf16(v[0], v[1]);
    o[1] = pack_bf16(v[2], v[3]);
    __builtin_amdgcn_raw_buffer_store_b64(o, r, voff, soff, 0);
}
// The lifetime / freshness bucket rule, stated once (lime_bucketize_f32, lime_bucketize_cuts_f32, lime_cached_occurrence_f32): the
// number of ascending fp32 cut points that are <= v.  cuts == nullptr: the nine cut points of num_buckets = 10, the smallest floats
// the reference's own fp32 evaluation of min(trunc(log(max(x, 1)) / log(86400) * (10 / 7)), 9) puts into buckets 1 .. 9
// (oracle/lime_oracle.py; tests/golden/bucket_edges.npz holds both neighbours of each).  A NaN compares false: bucket 0.
__device__ __forceinline__ int bucket_of(float v, const float* __restrict__ cuts, int n_cuts) {
    int b = 0;
    if (cuts == nullptr) {
        constexpr unsigned kBucketCuts[9] = {0x45326B18u, 0x4AF8B232u, 0x50AD53E8u, 0x567199BDu, 0x5C2861F4u,
                                     0x61EAB505u, 0x67A39429u, 0x6D6402D2u, 0x731EE960u};
#pragma unroll
        for (int k = 0; k < 9; ++k) b += (v >= __builtin_bit_cast(float, kBucketCuts[k])) ? 1 : 0;
    } else {
        for (int k = 0; k < n_cuts; ++k) b += (v >= cuts[k]) ? 1 : 0;
    }
    return b;
}

// Sum over the 16 lanes of a DPP row (the lanes that share a k slot, i.e. the 16 tokens of an MFMA tile): butterfly with quad_perm
// (xor 1, xor 2) and row rotations by 4 and 8; every lane ends up with the total.
__device__ __forceinline__ float row16_sum(float v) {
    int x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));        // quad_perm [1,0,3,2]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));        // quad_perm [2,3,0,1]
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, true));       // row_ror:4
    x = __builtin_bit_cast(int, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, true));       // row_ror:8
    return v;
}

}  // namespace lime_dev
