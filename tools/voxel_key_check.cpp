// mccnn_amd/csrc/voxel_key.h compiled for the host: the scalar half of the voxel accuracy against a table of cases.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/voxel_key_check.cpp -o voxel_key_check
//   ./voxel_key_check        exit status 0 and "ok <checks>" when all agree
// What is checked: the coordinate and its drop rule on and around every boundary (the minimum, -0.0f, 65535 / 65536, NaN, the
// infinities, points exactly on min + k res with res = 1 / 16 and with the float32 0.05), key packing and its fields, that no
// key is 0, the capacities, the validity rule against the integer form 10 g < 3 s, and a host run of the table itself --
// insert by the hash with linear probing into cap_min slots at a load of 0.9998 -- that finds every key in exactly one slot.
#include "voxel_key.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <set>
#include <vector>

using namespace mccnn;

static long checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s\n", __LINE__, #cond);                \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

struct CoordCase {
    float p, mn, res;
    bool kept;
    uint32_t v;
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float edge = 65535.0f / 16.0f;   // 4095.9375, exact
    const CoordCase table[] = {
        {1.0f, 1.0f, 0.05f, true, 0u},                       // on the minimum
        {0.98f, 1.0f, 0.05f, true, 0u},                      // a fraction of a voxel below it: ceilf gives -0.0f
        {0.94f, 1.0f, 0.05f, false, 0u},                     // more than a voxel below
        {1.0f + 0.0625f, 1.0f, 0.0625f, true, 1u},           // exactly on min + res
        {1.0f + 0.0626f, 1.0f, 0.0625f, true, 2u},
        {1.0f + 7 * 0.0625f, 1.0f, 0.0625f, true, 7u},
        {edge, 0.0f, 0.0625f, true, 65535u},                 // the last voxel
        {std::nextafterf(edge, 5000.0f), 0.0f, 0.0625f, false, 0u},
        {4096.0f, 0.0f, 0.0625f, false, 0u},                 // v = 65536
        {nan, 0.0f, 0.05f, false, 0u},       {0.0f, nan, 0.05f, false, 0u},
        {inf, 0.0f, 0.05f, false, 0u},       {-inf, 0.0f, 0.05f, false, 0u},
        {1.0f, -inf, 0.05f, false, 0u},      {1.0f, inf, 0.05f, false, 0u},
        {3.0e38f, -3.0e38f, 0.05f, false, 0u},               // the subtraction overflows
        {1.0e-30f, 0.0f, 0.05f, true, 1u},                   // anything above the minimum is voxel 1
        {0.05f, 0.0f, 0.05f, true, 1u},                      // 0.05f / 0.05f == 1
        {0.15f, 0.0f, 0.05f, true, 3u},                      // 0.15f / 0.05f rounds to 3.0f in float32 (3.0000000596 in double)
    };
    for (const CoordCase& c : table) {
        uint32_t v = 0xdeadu;
        const bool kept = voxel_coord(c.p, c.mn, c.res, v);
        EXPECT(kept == c.kept);
        if (kept) EXPECT(v == c.v);
    }
    // exactly on the grid with res = 1 / 16: v == k for every k
    for (uint32_t k = 0; k <= 65535u; ++k) {
        uint32_t v = 0;
        EXPECT(voxel_coord(-2.0f + (float)k * 0.0625f, -2.0f, 0.0625f, v) && v == k);
    }
    // with the float32 0.05 the rounded quotient decides: ceilf of the float32 division, whatever it is, and within one of k
    for (uint32_t k = 0; k <= 65535u; ++k) {
        const float p = (float)k * 0.05f;
        uint32_t v = 0;
        const float q = p / 0.05f;
        EXPECT(voxel_coord(p, 0.0f, 0.05f, v) == (ceilf(q) <= 65535.0f));
        if (ceilf(q) <= 65535.0f) EXPECT(v == (uint32_t)ceilf(q) && v + 1u >= k && v <= k + 1u);
    }

    // keys: fields, the occupied bit, never 0, distinct tuples give distinct keys
    EXPECT(voxel_key(0, 0, 0, 0) == (1ull << 63));
    EXPECT(voxel_key(32767u, 65535u, 65535u, 65535u) == 0xffffffffffffffffull);
    EXPECT(voxel_key(1, 2, 3, 4) == ((1ull << 63) | (1ull << 48) | (2ull << 32) | (3ull << 16) | 4ull));
    std::mt19937_64 rng(7);
    std::set<uint64_t> seen;
    std::set<std::vector<uint32_t>> tuples;
    for (int i = 0; i < 20000; ++i) {
        const uint32_t b = (uint32_t)(rng() % MCCNN_VOXEL_MAX_CLOUDS), x = (uint32_t)(rng() & 0xffff), y = (uint32_t)(rng() & 0xffff),
                       z = (uint32_t)(rng() & 0xffff);
        const uint64_t key = voxel_key(b, x, y, z);
        EXPECT(key != 0ull && (key >> 63) == 1ull && voxel_key_cloud(key) == b);
        EXPECT(((key >> 32) & 0xffff) == x && ((key >> 16) & 0xffff) == y && (key & 0xffff) == z);
        seen.insert(key);
        tuples.insert({b, x, y, z});
    }
    EXPECT(seen.size() == tuples.size());

    // capacities
    const uint64_t ns[] = {0, 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 100000, 600000, (1ull << 30) - 1};
    for (uint64_t n : ns) {
        const uint64_t rec = voxel_cap_rec(n), mn = voxel_cap_min(n);
        EXPECT((rec & (rec - 1)) == 0 && rec >= 64 && rec >= 2 * n && (rec == 64 || rec / 2 < 2 * n));
        EXPECT((mn & (mn - 1)) == 0 && mn > n && mn / 2 <= n && mn <= rec);
    }
    EXPECT(voxel_cap_rec(4095) == 8192 && voxel_cap_min(4095) == 4096 && voxel_cap_min(4096) == 8192);
    EXPECT(voxel_cap_rec((1ull << 30) - 1) == (1ull << 31) && voxel_slot_bytes(21) == 176);
    EXPECT(voxel_cap_rec(600000) * voxel_slot_bytes(21) == 369098752ull);

    // the validity rule: the double quotient against 10 g < 3 s
    for (uint32_t s = 1; s < 400; ++s)
        for (uint32_t g = 0; g <= s; ++g) {
            EXPECT(voxel_valid(g, s, 1, 0, 0.3) == (10 * g < 3 * s));
            EXPECT(!voxel_valid(g, s, 0, 0, 0.3));            // the majority is the ignore label
            EXPECT(voxel_valid(0, s, 0, -1, 0.3));             // no ignore label
        }
    EXPECT(!voxel_valid(0, 0, 1, 0, 0.3));

    // the table on the host: 4095 keys into cap_min = 4096 slots, every key in exactly one slot, chains that wrap the end
    {
        const uint64_t cap = voxel_cap_min(4095), mask = cap - 1;
        std::vector<uint64_t> keys(cap, 0ull);
        std::vector<uint32_t> rows(cap, 0u);
        uint64_t steps = 0, wrapped = 0;
        for (int pass = 0; pass < 2; ++pass)                   // the second pass finds what the first one claimed
            for (uint32_t i = 0; i < 4095u; ++i) {
                const uint64_t key = voxel_key(0, (i & 15u) + 1u, ((i >> 4) & 15u) + 1u, (i >> 8) + 1u);
                uint64_t s = voxel_hash(key) & mask;
                const uint64_t home = s;
                while (keys[s] != 0ull && keys[s] != key) {
                    s = (s + 1) & mask;
                    ++steps;
                    EXPECT(s != home);
                }
                if (s < home) ++wrapped;
                keys[s] = key;
                rows[s] += 1u;
            }
        uint64_t used = 0;
        for (uint64_t s = 0; s < cap; ++s) {
            EXPECT(rows[s] == (keys[s] ? 2u : 0u));
            used += keys[s] != 0ull;
        }
        EXPECT(used == 4095 && wrapped > 0);
        std::printf("full table: %.2f probe steps per insert, %llu chains wrapped\n", (double)steps / (2.0 * 4095.0),
                    (unsigned long long)wrapped);
    }
    // the hash spreads a room's worth of neighbouring voxels: at a load of 0.5 chains stay short
    {
        const uint64_t cap = 1ull << 18, mask = cap - 1;
        std::vector<uint64_t> keys(cap, 0ull);
        uint64_t steps = 0, n = 0;
        for (uint32_t x = 1; x <= 120; ++x)
            for (uint32_t y = 1; y <= 80; ++y)
                for (uint32_t z = 1; z <= 7; ++z) {
                    const uint64_t key = voxel_key(0, x, y, z);
                    uint64_t s = voxel_hash(key) & mask;
                    while (keys[s] != 0ull) { s = (s + 1) & mask; ++steps; }
                    keys[s] = key;
                    ++n;
                }
        std::printf("67200 voxels in 2^18 slots: %.3f probe steps per insert\n", (double)steps / (double)n);
        EXPECT((double)steps / (double)n < 1.0);
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
