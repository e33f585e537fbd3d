// claim_check -- the Cornell walk kernels' 32-bit pool arithmetic (mrt_launch.h pool_claim32,
// pool_tail32, pool_index32, pool_take32) against the 64-bit expressions of the path kernel's claim()
// that it replaces, stand-alone on the CPU for a sanitizer build (`make claim-check`: AddressSanitizer
// + UBSan, host code only, nothing preloaded; no GPU code runs).  Launches of 1 path up to the largest
// the host accepts (0xFFFFFFFF / npix whole samples, and 2^32 - 1 paths), partitioned by the render's own
// plan_partitions (mrt_plan.h) for each group shape the library builds; counter answers at a partition's start, at the launch's last path, around every
// edge (the partition's end, one claim before it, the tail zone's edge), past the partition's end and
// past 2^32; pools that hold 0, 1 and 63 paths when 1, 33 or 64 lanes take one, so that a claim
// straddles the pool and a partition's end.  Every result must agree exactly.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../miniraytracer_amd/csrc/mrt_plan.h"

using namespace mrtd;

static uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static unsigned long long g_checks = 0, g_bad = 0;

static void expect(bool ok, const char* what, uint64_t got, uint64_t pe, uint32_t batch, uint32_t have, uint32_t c, uint64_t a, uint64_t b) {
    g_checks++;
    if (ok) return;
    if (g_bad++ < 20)
        fprintf(stderr, "MISMATCH %s: got %llu pe %llu batch %u have %u c %u: 64-bit %llu, 32-bit %llu\n", what, (unsigned long long)got,
                (unsigned long long)pe, batch, have, c, (unsigned long long)a, (unsigned long long)b);
}

// one claim of c lanes from a pool [pool_next, pool_next + have) that falls short (have < c), or not
static void check(uint64_t got, uint32_t batch, uint64_t pe, uint32_t tail_zone, uint32_t n_paths, uint64_t pool_next, uint32_t have, uint32_t c) {
    // the 64-bit expressions (mrt_kernels.hip claim(), one try)
    uint64_t nb = 0, ne = 0, p_next = pool_next, p_end = pool_next + have;
    bool ok64 = false, tail64 = false;
    if (have < c) {
        nb = got;
        ok64 = nb < pe;
        if (ok64) {
            ne = umin64(nb + batch, pe);
            tail64 = pe - ne <= tail_zone / MRT_NPART;
        }
    }
    // the 32-bit ones
    uint32_t nb32 = 0, ne32 = 0, q_next = (uint32_t)pool_next, q_end = (uint32_t)(pool_next + have);
    bool ok32 = false, tail32 = false;
    if (have < c) {
        ok32 = pool_claim32(got, batch, (uint32_t)pe, &nb32, &ne32);
        if (ok32) tail32 = pool_tail32((uint32_t)pe, ne32, tail_zone);
    }
    expect(ok64 == ok32, "claimed", got, pe, batch, have, c, ok64, ok32);
    if (ok64 && ok32) {
        expect(nb == nb32 && ne == ne32, "claim's end", got, pe, batch, have, c, ne, ne32);
        expect(tail64 == tail32, "tail zone", got, pe, batch, have, c, tail64, tail32);
    }
    for (uint32_t r = 0; r < c; r++) {
        const uint64_t j = nb + (r - have);
        const uint64_t i64 = r < have ? pool_next + r : (j < ne ? j : ~0ull);
        const uint32_t i32 = have < c ? pool_index32(r, have, (uint32_t)pool_next, nb32, ne32) : (uint32_t)pool_next + r;
        expect((i64 < n_paths) == (i32 < n_paths), "a lane's path is valid", got, pe, batch, have, c, i64, i32);
        expect(i64 == ~0ull ? i32 == ~0u : i64 == i32, "a lane's path", got, pe, batch, have, c, i64, i32);
    }
    if (have < c) {
        p_next = umin64(nb + (c - have), ne);
        p_end = ne;
    } else {
        p_next += c;
    }
    pool_take32(c, have, nb32, ne32, &q_next, &q_end);
    expect(p_next == q_next && p_end == q_end, "the pool after", got, pe, batch, have, c, p_next, q_next);
    expect((p_next >= p_end) == (q_next >= q_end), "pool empty", got, pe, batch, have, c, p_next >= p_end, q_next >= q_end);
}

int main() {
    const uint32_t npix = 500u * 500u;
    const uint32_t launches[] = {1u, 63u, 64u, 129u, 500u, 8191u, 8193u, 8460u, 2099601u, 6759999u,
                                 0xFFFFFFFFu / npix * npix,  // the most whole samples of a 500 x 500 image
                                 0xFFFFFFFFu};
    // the three group shapes the library builds, each with its grid on 256 CUs: one-wave groups at eight
    // waves per SIMD, 4-wave groups at seven, the 12-wave treelet groups at six
    const struct { uint32_t waves; uint64_t grid; } shapes[] = {{1, 8192}, {4, 1792}, {12, 512}};
    for (const auto& shape : shapes)
    for (uint32_t n_paths : launches) {
        const uint64_t grid = shape.grid;
        // the partitions and tail zone of the launch as the render plans them (mrt_plan.h)
        PathParams P{};
        plan_partitions(P, n_paths, (int)grid, shape.waves);
        const uint32_t tail_zone = P.tail_zone;
        const uint64_t* const part_base = P.part_base;
        for (uint32_t k = 0; k < MRT_NPART; k++) {
            const uint64_t p0 = part_base[k], pe = part_base[k + 1];
            const uint64_t tz = tail_zone / MRT_NPART;
            for (uint32_t batch : {MRT_TAIL_BATCH, MRT_BATCH}) {
                std::vector<uint64_t> gots = {p0, p0 + 1, p0 + batch, pe, pe + 1, pe + batch, pe + (grid / MRT_NPART) * MRT_BATCH,
                                              0xFFFFFFFFull, 0x100000000ull, 0x100000000ull + p0, (1ull << 32) + pe, ~0ull >> 1};
                for (uint64_t d : {(uint64_t)1, (uint64_t)2, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)batch - 1, (uint64_t)batch,
                                   (uint64_t)batch + 1, tz, tz + 1, tz + batch - 1, tz + batch, tz + batch + 1})
                    if (pe >= d) gots.push_back(pe - d);  // (n_paths - 1, the launch's last path, is pe - 1 of the last partition)
                for (uint64_t got : gots)
                    for (uint32_t have : {0u, 1u, 63u, 64u, 200u})
                        for (uint32_t c : {1u, 33u, 64u}) {
                            // the pool's paths lie in this partition, or (a stolen claim) in the one before
                            for (uint64_t pool_next : {p0, pe >= have ? pe - have : 0, p0 >= 300u ? p0 - 300u : 0}) {
                                if (pool_next + have > n_paths) continue;
                                check(got, batch, pe, tail_zone, n_paths, pool_next, have, c);
                            }
                        }
            }
        }
    }
    printf("claim_check: %llu comparisons, %llu mismatches\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
