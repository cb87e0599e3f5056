// The codec of the packed copy of an fp32 X (rri_nmf_amd/csrc/rri_xpack.hpp) on the CPU, as a stand-alone program for the host
// compiler (tests/test_xpack_codec_cpu.py builds it with -fsanitize=address,undefined and runs it).  Exit status 0 and a last line
// "ok ..." when every check holds; the first failure is printed and ends the program with status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rri_xpack.hpp"

namespace xp = rri::xpack;

static int fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::printf("FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

// a small seeded generator (xorshift32): the sample of low parts
static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

// what the format says, written down independently of the header's arithmetic
static bool ref_in_window(uint32_t hi, uint32_t base) { return hi == 0 || (hi >= base && hi <= base + 14); }

int main() {
    const uint32_t bases[] = {1, 50, 113, 240};
    std::vector<uint32_t> los = {0u, 1u, 0x7fffffu, 0x800000u, 0xffffffu};
    for (int i = 0; i < 59; ++i) los.push_back(rnd() & 0xffffffu);
    unsigned long long checked = 0, flagged_count = 0;

    // 1. element by element: every top byte, every base; exact where in the window, flagged otherwise
    for (uint32_t base : bases)
        for (uint32_t hi = 0; hi < 256; ++hi)
            for (uint32_t lo : los) {
                const uint32_t b = hi << 24 | lo;
                const bool in = ref_in_window(hi, base);
                if (xp::in_window(b, base) != in) return fail("in_window", base, hi, lo);
                const uint32_t code = xp::encode_code(b, base);
                if (code > 15) return fail("code range", base, hi, code);
                if (in && xp::decode(lo, code, base) != b) return fail("decode(encode(b)) != b", base, hi, lo);
                if (in && (code == 15) != (hi == 0)) return fail("code 15 is the code of hi == 0 alone", base, hi, code);
                ++checked;
                flagged_count += !in;
            }

    // 2. whole lanes through encode_lane / decode_row: one element of interest in each of the 32 places, the rest a seeded
    //    in-window filling; the flag is raised exactly when that element is outside the window
    for (uint32_t base : bases)
        for (uint32_t hi = 0; hi < 256; ++hi)
            for (size_t li = 0; li < los.size(); ++li) {
                const int place = (int)((hi + li) % 32);
                uint32_t bits[xp::ROWS][xp::COLS], out[4 * xp::SLOTS], back[xp::COLS];
                for (int u = 0; u < 8; ++u)
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t r = rnd();
                        const uint32_t fh = (r >> 24) % 16 == 15 ? 0u : base + (r >> 24) % 15;   // zeros and every code
                        bits[u][e] = (fh > 255 ? 0u : fh) << 24 | (r & 0xffffffu);
                    }
                const uint32_t b = hi << 24 | los[li];
                bits[place / 4][place % 4] = b;
                bool all_in = true;
                for (int u = 0; u < 8; ++u)
                    for (int e = 0; e < 4; ++e) all_in = all_in && ref_in_window(bits[u][e] >> 24, base);
                bool flagged = false;
                xp::encode_lane(bits, base, out, flagged);
                if (flagged != !all_in) return fail("encode_lane flag", base, hi, los[li]);
                if (flagged) continue;
                for (int u = 0; u < 8; ++u) {
                    xp::decode_row(out, u, base * 0x01010101u, back);
                    for (int e = 0; e < 4; ++e)
                        if (back[e] != bits[u][e]) return fail("decode_row(encode_lane) differs", base, (unsigned)u * 4 + e, bits[u][e]);
                }
                // the dwords are the bytes the offsets name: lo byte j of (u, e) and its code, read back through the offsets
                const unsigned char* bytes = reinterpret_cast<const unsigned char*>(out);   // slot-major, 16 bytes per slot: lane 0 of
                for (int u = 0; u < 8; ++u)                                                  // a record with 1 lane per slot
                    for (int e = 0; e < 4; ++e) {
                        uint32_t lo = 0;
                        for (int j = 0; j < 3; ++j) {
                            const uint32_t off = xp::lo_byte_offset(0, u, e, j);
                            lo |= (uint32_t)bytes[off / xp::SLOT_BYTES * 16 + off % 16] << (8 * j);
                        }
                        const uint32_t coff = xp::code_byte_offset(0, u, e);
                        const uint32_t code = (bytes[coff / xp::SLOT_BYTES * 16 + coff % 16] >> xp::code_shift(e)) & 15u;
                        if (xp::decode(lo, code, base) != bits[u][e]) return fail("byte offsets disagree with encode_lane", base, u, e);
                    }
                ++checked;
            }

    // 3. the offsets of (lane, u, e, byte) and of the codes are a bijection onto the 7 KiB of a record, and records tile the copy
    {
        std::vector<int> hit(xp::RECORD_BYTES, 0);
        std::vector<int> nib(2 * xp::RECORD_BYTES, 0);
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t u = 0; u < 8; ++u)
                for (uint32_t e = 0; e < 4; ++e) {
                    for (uint32_t j = 0; j < 3; ++j) {
                        const uint32_t off = xp::lo_byte_offset(lane, u, e, j);
                        if (off >= 6 * xp::SLOT_BYTES) return fail("lo byte outside slots 0..5", lane, u, e);
                        hit[off] += 2;      // both nibbles of the byte
                    }
                    const uint32_t coff = xp::code_byte_offset(lane, u, e);
                    if (coff < 6 * xp::SLOT_BYTES || coff >= xp::RECORD_BYTES) return fail("code outside slot 6", lane, u, e);
                    nib[2 * coff + xp::code_shift(e) / 4] += 1;
                }
        for (uint32_t i = 0; i < xp::RECORD_BYTES; ++i) {
            const int n = i < 6 * xp::SLOT_BYTES ? hit[i] : nib[2 * i] + nib[2 * i + 1];
            if (n != 2) return fail("record byte not covered exactly once", i, (unsigned)n, 0);
            if (i >= 6 * xp::SLOT_BYTES && (nib[2 * i] != 1 || nib[2 * i + 1] != 1)) return fail("code nibble not covered exactly once", i, 0, 0);
        }
        if (xp::RECORD_BYTES != 7 * 1024) return fail("a record is 7 KiB", xp::RECORD_BYTES, 0, 0);
        const uint64_t panels = 12;
        std::vector<int> rec(5 * panels, 0);
        for (uint64_t q = 0; q < 5; ++q)
            for (uint64_t p = 0; p < panels; ++p) {
                const uint64_t off = xp::record_offset(q, p, panels);
                if (off % xp::RECORD_BYTES || off / xp::RECORD_BYTES >= rec.size()) return fail("record offset", q, p, off);
                rec[off / xp::RECORD_BYTES] += 1;
            }
        for (size_t i = 0; i < rec.size(); ++i)
            if (rec[i] != 1) return fail("records do not tile the copy", i, 0, 0);
        if (xp::record_offset(1, 4, panels) != xp::record_offset(1, 5, panels) - xp::RECORD_BYTES) return fail("panels of a chunk are adjacent", 0, 0, 0);
        // far beyond 2^32 bytes: 250000 chunks of 4000 panels
        if (xp::record_offset(250000, 3999, 4000) != (250000ull * 4000ull + 3999ull) * 7168ull) return fail("64-bit record offset", 0, 0, 0);
    }

    // 4. the window's base from the largest top byte
    for (uint32_t hmax = 0; hmax <= xp::HI_MAX; ++hmax) {
        const uint32_t want = hmax >= 15 ? hmax - 14 : 1;
        if (xp::base_of(hmax) != want) return fail("base_of", hmax, xp::base_of(hmax), want);
    }
    for (uint32_t hi = 0; hi < 256; ++hi) {
        const uint32_t want = (hi >= 1 && hi <= 0x7e) ? hi : 0;
        if (xp::window_candidate(hi << 24 | 0x123456u) != want) return fail("window_candidate", hi, 0, 0);
    }
    std::printf("ok %llu checks, %llu elements outside their window\n", checked, flagged_count);
    return 0;
}
