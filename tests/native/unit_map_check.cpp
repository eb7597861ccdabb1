// Host check of the expansion launch's work-unit map (rmc_units.h): counter
// value -> (window, quarter, first tile, tile count), and the units of a launch.
//   g++ -O2 -std=c++17 -I raft.tla_amd/csrc tests/native/unit_map_check.cpp -o unit_map_check && ./unit_map_check
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rmc_units.h"

using namespace rmc_units;

static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (++fails <= 20) {                        \
                printf("FAIL %s: ", #c);                \
                printf(__VA_ARGS__);                    \
                printf("\n");                           \
            }                                           \
        }                                               \
    } while (0)

int main() {
    const uint32_t ladder[] = {16, 8, 4, 2};
    uint64_t cases = 0, units = 0;
    for (uint32_t wt = 1; wt <= 16; ++wt) {
        const uint64_t W = 256ull * wt;
        const uint64_t nfs[] = {1, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, 3 * W + 77};
        for (uint32_t ut : ladder) {
            const uint32_t ng = unit_groups(wt, ut);
            CHECK(ng == (wt + ut - 1) / ut && ng >= 1, "wt %u ut %u ng %u", wt, ut, ng);
            for (uint64_t nf : nfs) {
                ++cases;
                const uint64_t total = units_total(nf, wt, ut);
                const uint64_t nwin = (nf + W - 1) / W;
                CHECK(total == nwin * 4 * ng, "wt %u ut %u nf %llu total %llu", wt, ut, (unsigned long long)nf,
                      (unsigned long long)total);
                // covered[(window * wt + tile) * 4 + quarter]: units with id < total that hold it
                std::vector<uint32_t> covered(nwin * wt * 4, 0);
                for (uint64_t id = 0; id < total; ++id) {
                    const Unit u = unit_decode((uint32_t)id, wt, ut, ng);
                    ++units;
                    CHECK(u.win < nf && u.win % W == 0, "wt %u ut %u nf %llu id %llu win %llu", wt, ut,
                          (unsigned long long)nf, (unsigned long long)id, (unsigned long long)u.win);
                    CHECK(u.quarter < 4 && u.ntiles >= 1 && u.ntiles <= ut && u.tile0 % ut == 0 &&
                              u.tile0 + u.ntiles <= wt,
                          "wt %u ut %u id %llu quarter %u tile0 %u ntiles %u", wt, ut, (unsigned long long)id,
                          u.quarter, u.tile0, u.ntiles);
                    if (u.win >= nf || u.quarter >= 4) continue;
                    for (uint32_t t = u.tile0; t < u.tile0 + u.ntiles && t < wt; ++t)
                        ++covered[((u.win / W) * wt + t) * 4 + u.quarter];
                    if (ut == 16)  // the units before tile groups: a wave's quarter of a whole window
                        CHECK(u.win == (id >> 2) * W && u.quarter == (id & 3) && u.tile0 == 0 && u.ntiles == wt,
                              "ut 16 wt %u id %llu", wt, (unsigned long long)id);
                }
                for (uint64_t w = 0; w < nwin; ++w) {
                    const uint64_t wn = nf - w * W < W ? nf - w * W : W;  // states in this window
                    for (uint32_t t = 0; t < wt; ++t)
                        for (uint32_t q = 0; q < 4; ++q) {
                            const uint32_t c = covered[(w * wt + t) * 4 + q];
                            if (t * 256ull + q * 64ull < wn)
                                CHECK(c == 1, "wt %u ut %u nf %llu window %llu tile %u quarter %u covered %u times", wt,
                                      ut, (unsigned long long)nf, (unsigned long long)w, t, q, c);
                            else
                                CHECK(c <= 1, "wt %u ut %u nf %llu window %llu tile %u quarter %u (empty) covered %u times",
                                      wt, ut, (unsigned long long)nf, (unsigned long long)w, t, q, c);
                        }
                }
                // every id from total on is past the launch: the next ones a resident grid can
                // draw, and the largest counter values
                for (uint64_t k = 0; k < 70000; ++k) {
                    const uint64_t id = k < 65536 ? total + k : 0xFFFFFFFFull - (k - 65536);
                    if (id < total || id > 0xFFFFFFFFull) continue;
                    const Unit u = unit_decode((uint32_t)id, wt, ut, ng);
                    CHECK(u.win >= nf, "wt %u ut %u nf %llu id %llu >= total %llu decodes to win %llu", wt, ut,
                          (unsigned long long)nf, (unsigned long long)id, (unsigned long long)total,
                          (unsigned long long)u.win);
                    CHECK(u.tile0 + u.ntiles <= wt, "wt %u ut %u id %llu past the window's tiles", wt, ut,
                          (unsigned long long)id);
                }
            }
        }
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok %llu cases, %llu units\n", (unsigned long long)cases, (unsigned long long)units);
    return 0;
}
