// rmc_dev_outbox.h — sharded mode: a rank's key outboxes and its parking buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "rmc_internal.h"

namespace rmc {

// Phase-1 keys travel as the raw fingerprint (k, low 32 bits of s): the owner
// derives its own table value and slot (tkey; tables may differ in size across
// ranks).  Outbox: 12 B per key, three u32 {k lo, k hi, s32} (round 6; 16 B
// before: a quarter of phase 1's bytes was padding); parking (B.ovf): {k, s32 | flags << 32,
// ticket}, where flag OVF_UNKEYED marks a ticket the expansion parked without
// computing its key (k_route_fix computes it).
constexpr u64 OVF_UNKEYED = 1ull << 32;
__device__ __forceinline__ void put_key(const DevBufs& B, u32 dest, u64 slot, u64 k, u32 s32, u64 tick) {
    u32* o = reinterpret_cast<u32*>(B.key_out) + 3 * ((u64)dest * B.kcap + slot);
    o[0] = (u32)k;
    o[1] = (u32)(k >> 32);
    o[2] = s32;
    B.tick_out[(u64)dest * B.kcap + slot] = tick;
}
__device__ __forceinline__ void park_key(const DevBufs& B, u64 k, u64 s_and_flags, u64 tick) {
    const u64 q = atomicAdd((unsigned long long*)&B.ctr->novf, 1ull);
    if (q < B.ovf_cap) {
        B.ovf[3 * q] = k;
        B.ovf[3 * q + 1] = s_and_flags;
        B.ovf[3 * q + 2] = tick;
    } else {
        atomicOr(&B.ctr->overflow, 2u);  // the parking buffer is full too: fatal
    }
}

}  // namespace rmc
