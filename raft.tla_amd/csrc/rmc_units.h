// rmc_units.h — the dynamic work units of an expansion launch over presorted
// windows (expand_body, DYN): how a value of the launch's work counter
// (Counters.wnext) names a wave's work.  A unit is (window, quarter, tile
// group): the 64 positions `quarter * 64 ..` of the tiles
// `tile0 .. tile0 + ntiles - 1` of one window of `wt` tiles of 256 positions;
// a group is `ut` tiles (a power of two, at most 16), the last one of a window
// the `wt % ut` that remain.  The quarter varies fastest, then the group, then
// the window: the four quarters of one tile group are claimed back to back.
// With ut = 16 a unit is a wave's quarter of a whole window,
// (id >> 2, id & 3, 0, wt).  Arithmetic only (no HIP includes), shared by the
// kernel and the host test (tests/native/unit_map_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RMC_UNITS_HD __host__ __device__
#else
#define RMC_UNITS_HD
#endif

namespace rmc_units {

struct Unit {
    uint64_t win;     // the window's first position in the launch (>= nf: past the launch's last unit)
    uint32_t quarter; // 0..3: positions quarter * 64 .. + 63 of every tile
    uint32_t tile0;   // first tile
    uint32_t ntiles;  // tiles (tile0 + ntiles <= wt)
};

// tile groups per quarter of a window of wt tiles
RMC_UNITS_HD inline uint32_t unit_groups(uint32_t wt, uint32_t ut) { return (wt + ut - 1) / ut; }

// The unit of counter value `id`; ng = unit_groups(wt, ut), launch-uniform.
RMC_UNITS_HD inline Unit unit_decode(uint32_t id, uint32_t wt, uint32_t ut, uint32_t ng) {
    const uint32_t r = id >> 2, w = r / ng, g = r - w * ng;
    Unit u;
    u.win = (uint64_t)w * 256ull * wt;
    u.quarter = id & 3u;
    u.tile0 = g * ut;
    u.ntiles = wt - u.tile0 < ut ? wt - u.tile0 : ut;
    return u;
}

// Admission (rmc_plan.h): Counters.wnext carries this bit once a flush has taken the count
// past the launch's stop; a claim that returns it names no unit (it decodes to a window past
// any launch: a launch has fewer than 2^24 units) and is taken back, so the bits below it
// stay the units claimed.
constexpr uint32_t kStopBit = 0x80000000u;
RMC_UNITS_HD inline uint64_t units_claimed(uint64_t wnext) { return wnext & (kStopBit - 1u); }

// Units of a launch of nf states: every id below it names a unit of a window
// that starts inside the launch, every id from it on decodes to win >= nf.
RMC_UNITS_HD inline uint64_t units_total(uint64_t nf, uint32_t wt, uint32_t ut) {
    const uint64_t nwin = (nf + 256ull * wt - 1) / (256ull * wt);
    return nwin * 4ull * unit_groups(wt, ut);
}

}  // namespace rmc_units
