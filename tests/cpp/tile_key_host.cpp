// tile_key_host.cpp -- the pair <-> (entry, bit) map of the tile lists (csrc/cvo_device.h tile_pair / tile_key) on the CPU.
//
// expand_lists turns bit `bit` of a TileEntry (x, y) into the pair tile_pair(x, y, bit); k_tiles_from_record goes the other way,
// tile_key(i, j), when it rebuilds a list from its candidate record.  Checked here:
//   1. for every result register r, every bit 0 .. 63 and tiles that begin at rows / columns 0, 16 and the last tile of clouds of
//      10 000 and of 65 536 rows: pair -> (entry, bit) -> pair is the identity, and so is (entry, bit) -> pair -> (entry, bit);
//   2. an entry rebuilt from a subset of its 64 pairs (the OR of their bits: every one of them names the same entry) expands to
//      exactly that subset -- every single pair, every two pairs, the full entry, and 4 000 random subsets per entry;
//   3. pairs of different entries never share a key: the 16 x 16 pairs of a tile fall into its four entries, 64 each.
// Prints "ok" and returns 0 when all of it holds.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "cvo_device.h"

using namespace cvo_dev;

namespace {

int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (fails < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++fails;                                       \
        }                                                  \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd64()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// the pairs a mask of entry (x, y) expands to, as expand_lists makes them
std::set<std::pair<unsigned, unsigned>> expand(unsigned x, unsigned y, uint64_t mask)
{
    std::set<std::pair<unsigned, unsigned>> out;
    for (unsigned bit = 0; bit < 64; ++bit)
        if ((mask >> bit) & 1ull) {
            unsigned i, j;
            tile_pair(x, y, bit, i, j);
            out.insert({i, j});
        }
    return out;
}

// the entry rebuilt from a set of pairs that must all name entry (x, y)
uint64_t rebuild(unsigned x, unsigned y, const std::set<std::pair<unsigned, unsigned>> &pairs)
{
    uint64_t m = 0;
    for (const auto &p : pairs) {
        unsigned kx, ky, bit;
        tile_key(p.first, p.second, kx, ky, bit);
        CHECK(kx == x && ky == y, "pair (%u, %u) of entry (%u, %#x) names entry (%u, %#x)", p.first, p.second, x, y, kx, ky);
        CHECK(bit < 64 && !((m >> bit) & 1ull), "pair (%u, %u): bit %u twice", p.first, p.second, bit);
        m |= 1ull << bit;
    }
    return m;
}

void one_tile(unsigned row0, unsigned col0)
{
    std::set<std::pair<unsigned, unsigned>> seen;   // every pair of the tile, over its four entries
    for (unsigned r = 0; r < 4; ++r) {
        const unsigned x = row0, y = col0 | (r << 30);
        for (unsigned bit = 0; bit < 64; ++bit) {
            unsigned i, j;
            tile_pair(x, y, bit, i, j);
            // (what the filter's ballot says of the bit: row (bit >> 4) * 4 + r, column bit & 15 of the tile)
            CHECK(i == row0 + (bit >> 4) * 4 + r && j == col0 + (bit & 15), "tile (%u, %u) r %u bit %u -> (%u, %u)", row0, col0, r, bit, i, j);
            CHECK(i < 65536u && j < 65536u, "tile (%u, %u) r %u bit %u leaves the 16-bit rows", row0, col0, r, bit);
            unsigned kx, ky, kb;
            tile_key(i, j, kx, ky, kb);
            CHECK(kx == x && ky == y && kb == bit, "tile (%u, %u) r %u bit %u -> (%u, %u) -> (%u, %#x, %u)", row0, col0, r, bit, i, j, kx, ky, kb);
            unsigned i2, j2;
            tile_pair(kx, ky, kb, i2, j2);
            CHECK(i2 == i && j2 == j, "pair (%u, %u) -> key -> (%u, %u)", i, j, i2, j2);
            CHECK(seen.insert({i, j}).second, "pair (%u, %u) in two entries", i, j);
            // single pairs
            const auto one = expand(x, y, 1ull << bit);
            CHECK(one.size() == 1 && rebuild(x, y, one) == (1ull << bit), "tile (%u, %u) r %u: single bit %u", row0, col0, r, bit);
        }
        // every two pairs
        for (unsigned b0 = 0; b0 < 64; ++b0)
            for (unsigned b1 = b0 + 1; b1 < 64; ++b1) {
                const uint64_t m = (1ull << b0) | (1ull << b1);
                const auto s = expand(x, y, m);
                CHECK(s.size() == 2 && rebuild(x, y, s) == m && expand(x, y, rebuild(x, y, s)) == s, "tile (%u, %u) r %u: bits %u %u", row0, col0, r, b0, b1);
            }
        // the full entry and random subsets
        for (int t = 0; t < 4001; ++t) {
            uint64_t m = t == 0 ? ~0ull : rnd64();
            if (t % 3 == 1) m &= rnd64();          // sparse
            if (t % 3 == 2) m |= rnd64();          // dense
            if (m == 0) m = 1;
            const auto s = expand(x, y, m);
            const uint64_t back = rebuild(x, y, s);
            CHECK(s.size() == (size_t)__builtin_popcountll(m) && back == m, "tile (%u, %u) r %u: mask %#llx came back %#llx", row0, col0, r,
                  (unsigned long long)m, (unsigned long long)back);
            CHECK(expand(x, y, back) == s, "tile (%u, %u) r %u: mask %#llx expands to another set", row0, col0, r, (unsigned long long)m);
        }
    }
    CHECK(seen.size() == 256, "tile (%u, %u): %zu pairs in its four entries", row0, col0, seen.size());
    for (unsigned di = 0; di < 16; ++di)
        for (unsigned dj = 0; dj < 16; ++dj) CHECK(seen.count({row0 + di, col0 + dj}) == 1, "tile (%u, %u): pair (+%u, +%u) missing", row0, col0, di, dj);
}

}   // namespace

int main()
{
    // first rows / columns: 0, 16, the last tile of 10 000 rows (9 984) and of 65 536 rows (65 520)
    const unsigned firsts[] = {0u, 16u, (10000u - 1u) & ~15u, 65536u - 16u};
    for (unsigned row0 : firsts)
        for (unsigned col0 : firsts) one_tile(row0, col0);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
