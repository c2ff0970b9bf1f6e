// Inter-workgroup hand-offs of the multi-workgroup recurrences (lstm.hip, gru.hip, melar.hip, wavernn_tile.hip) — device side.
//
// Granule protocol.  Every exchanged value is an 8-byte granule {fp32 value, step tag} written with ONE agent-scope store, so payload and
// "it has arrived" can never be seen apart: no separate flag or counter, no producer-side drain.  A consumer lane polls the granules it needs
// until they carry the tag of the step.  Tags start at 1; the areas are zeroed before a launch (the host side re-arms them, see HandoffArea in
// common.hpp and the launchers).  Buffers are a ring of two slots by step parity: a member overwrites the step-t granule only at step t + 2,
// which it cannot reach before every member has published step t + 1, i.e. has consumed step t — two slots suffice.
// (tools/probes/handoff_probe.hip: 0.75 us per hand-off with agent-scope accesses, same or different XCD; workgroup-scope accesses are NOT
// coherent across CUs.)
//
// Counter protocol (g_st / g_ld / g_publish / g_wait).  Payload: agent-scope relaxed atomic stores / loads (write-through, L1-bypassing);
// arrival: every storing wave drains vmcnt(0), one lane bumps a monotonic counter; consumers poll it from one lane.
//
// Abort.  Every spin is bounded: a member that is not resident must not hang the GPU.  A poll that runs out of passes, or that sees the abort
// word set by another member, sets abort_word[0] (this launch: the other members stop at their next look) and returns false; the caller leaves
// the kernel.  The LSTM / GRU / mel-AR areas keep a sticky copy in abort_word[1] that survives the re-arm of the next launch until
// handoff_status() has reported it (GS_SPIN_LIMIT, STICKY = true); the WaveRNN handle reads the abort word of its own launch and has no
// sticky copy (WT_SPIN_LIMIT, STICKY = false).
#pragma once
#include <hip/hip_runtime.h>

namespace ttsc {

constexpr unsigned GS_SPIN_LIMIT = 1u << 22;   // split LSTM / GRU / mel-AR recurrences
constexpr unsigned WT_SPIN_LIMIT = 1u << 20;   // WaveRNN tile decode

typedef unsigned long long u64;                               // one granule: value in the low half, tag in the high half
typedef float f32x2 __attribute__((ext_vector_type(2)));   // packed pair of the resident-weight kernels (v_pk_fma_f32)

__device__ __forceinline__ u64 granule_tag(unsigned tag) { return (u64)tag << 32; }
// (tg = granule_tag(..): the sites that store several values under one tag)
__device__ __forceinline__ void st_granule_word(u64* p, float v, u64 tg) {
    __hip_atomic_store(p, tg | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_granule(u64* p, float v, unsigned tag) { st_granule_word(p, v, granule_tag(tag)); }
__device__ __forceinline__ float granule_value(u64 g) { return __uint_as_float((unsigned)g); }

// have all granules of `mask` arrived: do their bits from TAG_SHIFT upwards equal `tag`?  (A function with early returns on purpose: with the
// tags and-ed into a flag inside the spin loop hipcc emits a spin loop with more mask bookkeeping per pass: measured +2 % on the two-layer WaveRNN step
// and on the batched BiLSTM(256) step.)
template <int TAG_SHIFT, int N>
__device__ __forceinline__ bool granules_tagged(const u64 (&g)[N], unsigned mask, unsigned tag) {
#pragma unroll
    for (int r = 0; r < N; ++r)
        if ((mask >> r & 1u) && (unsigned)(g[r] >> TAG_SHIFT) != tag) return false;
    return true;
}

// THE poll: up to N granules per thread (src[off[r]] for the r set in `mask`) in ONE round trip — every load is issued before the first tag is
// looked at, and a pass is repeated only while some granule is missing (granule by granule the L2 round trip is paid once per granule even
// when all of them have arrived).  A granule has arrived when its bits from TAG_SHIFT upwards equal `tag` (32: the whole tag half; WaveRNN's
// candidate granule keeps a class index in the low byte of the tag half and polls with 40).  The abort word is looked at every 64th pass.
// false after LIMIT passes or when another member aborted; g[] then holds what the last pass saw.
template <unsigned LIMIT, bool STICKY, int TAG_SHIFT = 32, int N>
__device__ __forceinline__ bool poll_granules(const u64* src, const int (&off)[N], unsigned mask, unsigned tag, unsigned* abort_word, u64 (&g)[N]) {
    unsigned spins = 0;
    for (;;) {
#pragma unroll
        for (int r = 0; r < N; ++r)
            if (mask >> r & 1u) g[r] = __hip_atomic_load(src + off[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (granules_tagged<TAG_SHIFT>(g, mask, tag)) return true;
        if (++spins > LIMIT || ((spins & 63u) == 0u && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (STICKY) __hip_atomic_store(abort_word + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sticky copy (common.hpp HandoffArea)
            return false;
        }
        __builtin_amdgcn_s_sleep(1);   // (longer back-offs only add latency: measured 18.1 / 18.7 / 20.8 us per WaveRNN step for 0 / 1k / 4k clocks)
    }
}

// the same, values scattered to out[dst[r]] (nothing is written after a failure)
template <unsigned LIMIT, bool STICKY, int N>
__device__ __forceinline__ bool poll_granules_to(const u64* src, const int (&off)[N], const int (&dst)[N], unsigned mask, unsigned tag, unsigned* abort_word,
                                                 float* out) {
    u64 g[N];
    if (!poll_granules<LIMIT, STICKY>(src, off, mask, tag, abort_word, g)) return false;
#pragma unroll
    for (int r = 0; r < N; ++r)
        if (mask >> r & 1u) out[dst[r]] = granule_value(g[r]);
    return true;
}

// the same for the N granules p[i * stride], values to v[i] (after a failure: what the last pass saw)
template <unsigned LIMIT, bool STICKY, int N>
__device__ __forceinline__ bool poll_granules_strided(const u64* p, int stride, unsigned tag, unsigned* abort_word, float (&v)[N]) {
    u64 g[N];
    int off[N];
#pragma unroll
    for (int i = 0; i < N; ++i) off[i] = i * stride;
    const bool ok = poll_granules<LIMIT, STICKY>(p, off, (1u << N) - 1u, tag, abort_word, g);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = granule_value(g[i]);
    return ok;
}

// ---- counter protocol -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void g_st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float g_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool g_wait(unsigned* cnt, unsigned want, unsigned* abort_word, int* ok_s) {
    if (threadIdx.x == 0) {
        int ok = 1;
        unsigned spins = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
            if (++spins > GS_SPIN_LIMIT || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(abort_word + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sticky copy (common.hpp HandoffArea)
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        *ok_s = ok;
    }
    __syncthreads();
    return *ok_s != 0;
}
__device__ __forceinline__ void g_publish(unsigned* cnt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace ttsc
