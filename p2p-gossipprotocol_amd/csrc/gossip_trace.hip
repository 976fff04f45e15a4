// gossip_trace.hip -- receipt trace (GOSSIP_FLAG_RECEIPT_TRACE): the round in which
// every owned (peer, message) pair was first received, and every owned peer's death round, kept on the device.
//
// k_trace_receipts runs once per round, after everything that can add a receipt and before the word buffers
// rotate (advance(), gossip_engine.hip).  It does not trust the round's "next new words" buffer to be exact
// (pull rounds leave stale words in it, list rounds clear theirs lazily, deferred rounds keep their receipts
// nowhere else): it compares seen (OR the deferred round's words) against a shadow of what the trace has
// already recorded, so a stale bit is a bit the shadow holds and costs nothing.
#include <hip/hip_runtime.h>

#include "gossip_device.hpp"
#include "gossip_internal.hpp"

namespace gossip {
namespace {

// One wave per 64-peer tile.  Lane l loads the words of peer tile * 64 + l (coalesced), the fresh bits are
// seen & ~shadow; a ballot finds the peers with any, and for each of them the fresh word is broadcast and
// lane m stores the round into entry m of that peer's row: one contiguous 128-B store per (peer, word) with
// receipts, nothing but the loads for a tile without.  LANES = true is the A/B shape (each lane walks the
// bits of its own peer and stores into its own row: 64 rows per store instruction).
template <bool LANES>
__global__ __launch_bounds__(kBlock) void k_trace_receipts(const TraceArgs t) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t tiles = (t.n_local + 63) / 64;
    const uint16_t r = (uint16_t)t.round;
    for (uint64_t tile = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6); tile < tiles; tile += waves) {
        const uint64_t v = tile * 64 + lane;
        const bool in = v < t.n_local;
        if (in && !bit_alive(t.alive, (uint32_t)(t.begin + v)) && t.death[v] == GOSSIP_NEVER) t.death[v] = r;
        for (uint32_t w = 0; w < t.W; ++w) {
            uint64_t fresh = 0;
            if (in) {
                const uint64_t i = v * t.Wp + w;
                uint64_t cur = t.seen[i];
                if (t.extra) cur |= t.extra[i];
                const uint64_t old = t.shadow[i];
                fresh = cur & ~old;
                if (fresh) t.shadow[i] = old | fresh;
            }
            if (LANES) {
                while (fresh) {
                    const uint32_t m = w * 64 + (uint32_t)__builtin_ctzll(fresh);
                    fresh &= fresh - 1;
                    if (m < t.M) t.receipt[v * t.M + m] = r;
                }
            } else {
                unsigned long long has = __ballot(fresh != 0);
                const uint32_t m = w * 64 + lane;
                while (has) {
                    const int src = __builtin_ctzll(has);
                    has &= has - 1;
                    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)fresh, src);
                    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(fresh >> 32), src);
                    const uint64_t f = ((uint64_t)hi << 32) | lo;
                    // (src had fresh bits, so tile * 64 + src < n_local; m < M keeps the store inside its row)
                    if (((f >> lane) & 1ull) && m < t.M) t.receipt[(tile * 64 + (uint64_t)src) * t.M + m] = r;
                }
            }
        }
    }
}

// hist[r * M + m] += entries of message m equal to r, r < rounds.  LDS = true: rounds * M u32 bins per
// workgroup in dynamic LDS, flushed with one 64-bit atomic per nonzero bin; false: global atomics.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_trace_hist(const uint16_t* receipt, uint64_t entries, uint32_t M,
                                                       uint32_t rounds, unsigned long long* hist) {
    extern __shared__ uint32_t bins[];
    const uint32_t nb = rounds * M;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) bins[i] = 0;
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto count = [&](uint32_t r, uint32_t m) {
        if (r < rounds) {
            if (LDS) atomicAdd(&bins[r * M + m], 1u);
            else atomicAdd(&hist[r * M + m], 1ull);
        }
    };
    // 16-B loads of eight entries (the array starts on an allocation boundary), then the tail
    const uint64_t n8 = entries / 8;
    const uint4* r4 = reinterpret_cast<const uint4*>(receipt);
    for (uint64_t i = tid; i < n8; i += stride) {
        const uint4 x = r4[i];
        const uint32_t wd[4] = {x.x, x.y, x.z, x.w};
        uint32_t m = (uint32_t)((i * 8) % M);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            count((wd[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu, m);
            if (++m == M) m = 0;
        }
    }
    for (uint64_t i = n8 * 8 + tid; i < entries; i += stride) count(receipt[i], (uint32_t)(i % M));
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x)
            if (bins[i]) atomicAdd(&hist[i], (unsigned long long)bins[i]);
    }
}

}  // namespace

hipError_t launch_trace_receipts(const TraceArgs& t, hipStream_t s) {
    const uint64_t tiles = (t.n_local + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>((tiles + kWavesPerBlock - 1) / kWavesPerBlock, kMaxGrid * 4ull);
    if (!grid) return hipSuccess;
    if (t.shape == 1) hipLaunchKernelGGL(k_trace_receipts<true>, dim3(grid), dim3(kBlock), 0, s, t);
    else hipLaunchKernelGGL(k_trace_receipts<false>, dim3(grid), dim3(kBlock), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_trace_hist(const uint16_t* receipt, uint64_t n_local, uint32_t M, uint32_t rounds,
                             unsigned long long* hist, hipStream_t s) {
    const uint64_t entries = n_local * M;
    if (!entries || !rounds) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((entries + kBlock - 1) / kBlock, kMaxGrid);
    const uint64_t nb = (uint64_t)rounds * M;
    if (nb <= kTraceHistLds)
        hipLaunchKernelGGL(k_trace_hist<true>, dim3(grid), dim3(kBlock), nb * sizeof(uint32_t), s, receipt, entries, M,
                           rounds, hist);
    else
        hipLaunchKernelGGL(k_trace_hist<false>, dim3(grid), dim3(kBlock), 0, s, receipt, entries, M, rounds, hist);
    return hipGetLastError();
}

}  // namespace gossip
