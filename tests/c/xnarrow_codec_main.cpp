// The codec of the 26-bit copy of an fp32 X (rri_nmf_amd/csrc/rri_xnarrow.hpp) on the CPU, as a stand-alone program for the host
// compiler (tests/test_xnarrow_codec_cpu.py builds it with -fsanitize=address,undefined and runs it).  Exit status 0 and a last
// line "ok ..." when every check holds; the first failure is printed and ends the program with status 1.
//
// A record is encoded the way k_xnarrow_encode does it (encode_lane per lane, the entries lane after lane) and decoded the way
// the row loop of k_pass does it: the entries go through map_offset into a byte map of 8 rows x 64 dwords, rare_entry gives the
// exponent byte, and decode_row takes the lane's 26 dwords, the book and the map dword of its row.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rri_xnarrow.hpp"

namespace xn = rri::xnarrow;
namespace xp = rri::xpack;

static int fail(const char* what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::printf("FAILED: %s (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

struct Record {
    std::vector<uint32_t> fixed;       // the 6.5 KiB, as the bytes of the record
    std::vector<uint16_t> entries;
    bool neither = false;
};
typedef uint32_t LaneBits[xn::ROWS][xn::COLS];

// the encoder of a record: x[lane] = the lane's 8 x 4 elements
static Record encode_record(const std::vector<uint32_t>& x, const uint8_t (&cls)[256], uint32_t rows_valid) {
    Record r;
    r.fixed.assign(xn::RECORD_BYTES / 4, 0u);
    for (uint32_t lane = 0; lane < xn::LANES; ++lane) {
        LaneBits bits;
        std::memcpy(bits, &x[lane * xn::ELEMS], sizeof(bits));
        uint32_t out[xn::LANE_DWORDS], nexc = 0, again = 0;
        uint16_t exc[xn::ELEMS];
        bool neither = false, neither2 = false;
        xn::encode_lane(bits, rows_valid, cls, lane, out, nullptr, nexc, neither);       // the counting call
        if (nexc > xn::ELEMS) { r.neither = true; return r; }
        xn::encode_lane(bits, rows_valid, cls, lane, out, exc, again, neither2);
        if (again != nexc || neither != neither2) { std::printf("FAILED: the counting call and the writing call differ\n"); std::exit(1); }
        r.neither = r.neither || neither;
        for (uint32_t k = 0; k < xn::LANE_DWORDS; ++k) r.fixed[xn::dword_offset(k, lane) / 4] = out[k];
        r.entries.insert(r.entries.end(), exc, exc + nexc);
    }
    return r;
}
// the decoder of a record, as the pass goes about it; the map is cleared, filled, read
static void decode_record(const Record& r, const xn::Books& books, std::vector<uint32_t>& x) {
    const uint32_t MAP_ROW = 72 * 8;
    std::vector<unsigned char> map(8 * MAP_ROW, 0xa5);       // the tile holds row sums when a chunk starts
    for (uint32_t u = 0; u < 8; ++u)
        for (uint32_t lane = 0; lane < 64; ++lane) std::memset(&map[u * MAP_ROW + 4 * lane], 0, 4);
    for (uint32_t first = 0; first < 64 && first < r.entries.size(); ++first)            // lanes take entries lane, lane + 64, ...
        for (size_t j = first; j < r.entries.size(); j += 64) {
            const uint32_t en = r.entries[j];
            map[xn::map_offset(en & 2047u, MAP_ROW)] = (unsigned char)xn::rare_entry(books, en >> xn::POS_BITS);
        }
    x.assign(xn::LANES * xn::ELEMS, 0u);
    for (uint32_t lane = 0; lane < xn::LANES; ++lane) {
        uint32_t in[xn::LANE_DWORDS];
        for (uint32_t k = 0; k < xn::LANE_DWORDS; ++k) in[k] = r.fixed[xn::dword_offset(k, lane) / 4];
        for (int u = 0; u < 8; ++u) {
            uint32_t mapped, back[xn::COLS];
            std::memcpy(&mapped, &map[(uint32_t)u * MAP_ROW + 4 * lane], 4);
            xn::decode_row(in, u, mapped, books.lo, books.hi, back);
            for (int e = 0; e < 4; ++e) x[lane * xn::ELEMS + 4 * u + e] = back[e];
        }
    }
}

// books for a window of `base` in which exponent byte `eb` is in the book (0), only in the rare book (1): a histogram that puts
// it first, or last, among the candidates
static uint64_t books_with(uint32_t base, uint32_t eb, int where, xn::Books& b, uint8_t (&cls)[256], int& nrare) {
    uint64_t hist[256] = {};
    for (uint32_t e = 0; e < 256; ++e) hist[e] = 1000 + (e * 37u) % 101u;
    hist[eb] = where == 0 ? 1000000 : 1;
    return xn::choose_books(hist, base, b, cls, nrare);
}

int main() {
    const uint32_t bases[] = {1, 50, 112};
    std::vector<uint32_t> mants = {0u, 1u, 0x3fffffu, 0x400000u, 0x7fffffu};
    for (int i = 0; i < 11; ++i) mants.push_back(rnd() & 0x7fffffu);
    unsigned long long checked = 0, reported = 0;

    // 1. every exponent byte x books that hold it in the book, only in the rare book, or nowhere (bytes outside the window are in
    //    neither, whatever the histogram): the element of interest in a rotating place of a rotating lane, the rest a seeded
    //    filling from both books
    for (uint32_t base : bases)
        for (uint32_t eb = 0; eb < 256; ++eb)
            for (int where = 0; where < 2; ++where) {
                xn::Books books;
                uint8_t cls[256];
                int nrare = 0;
                books_with(base, eb, where, books, cls, nrare);
                const bool in = xp::in_window(eb << 23, base);
                if (in && (where == 0) != (cls[eb] < xn::BOOK)) return fail("the histogram did not place the byte", base, eb, where);
                if (!in && cls[eb] != xn::CLS_NONE) return fail("a byte outside the window is in a book", base, eb, cls[eb]);
                std::vector<uint32_t> members;
                for (uint32_t e = 0; e < 256; ++e)
                    if (cls[e] != xn::CLS_NONE) members.push_back(e);
                for (size_t mi = 0; mi < mants.size(); ++mi) {
                    std::vector<uint32_t> x(xn::LANES * xn::ELEMS), back;
                    for (uint32_t& v : x) {
                        const uint32_t r = rnd();
                        v = members[(r >> 23) % members.size()] << 23 | (r & 0x7fffffu);
                    }
                    const uint32_t place = (eb * 31u + (uint32_t)mi * 7u + (uint32_t)where) % (xn::LANES * xn::ELEMS);
                    x[place] = eb << 23 | mants[mi];
                    const Record rec = encode_record(x, cls, 8);
                    if (rec.neither != !in) return fail("an element in neither book must be reported, and only that", base, eb, mants[mi]);
                    reported += rec.neither;
                    ++checked;
                    if (rec.neither) continue;
                    decode_record(rec, books, back);
                    for (size_t i = 0; i < x.size(); ++i)
                        if (back[i] != x[i]) return fail("decode(encode(x)) differs", base, i, x[i]);
                }
            }
    // a negative element is in neither book
    {
        xn::Books books;
        uint8_t cls[256];
        int nrare = 0;
        books_with(112, 253, 0, books, cls, nrare);
        std::vector<uint32_t> x(xn::LANES * xn::ELEMS, 0x3f800000u);
        x[77] = 0xbf800000u;
        if (!encode_record(x, cls, 8).neither) return fail("a negative element must be reported", 0, 0, 0);
        x[77] = 0x80000000u;
        if (!encode_record(x, cls, 8).neither) return fail("-0 must be reported", 0, 0, 0);
    }

    // 2. records with 0, 1, 63, 64, 65 and 2048 exceptions, the first and the last position among them; padding rows
    {
        xn::Books books;
        uint8_t cls[256];
        int nrare = 0;
        uint64_t hist[256] = {};
        for (uint32_t e = 224; e < 254; ++e) hist[e] = e;            // the window of base 112: bytes 224..253 (and 0, 1)
        hist[0] = 300;                                                // zeros: the most frequent
        xn::choose_books(hist, 112, books, cls, nrare);
        if (nrare != 25 || cls[0] != 0 || cls[253] != 1 || cls[1] != xn::CLS_RARE + 24) return fail("books of a plain histogram", nrare, cls[0], cls[1]);
        std::vector<uint32_t> bookv, rarev;
        for (uint32_t e = 0; e < 256; ++e) {
            if (cls[e] < xn::BOOK) bookv.push_back(e);
            else if (cls[e] != xn::CLS_NONE) rarev.push_back(e);
        }
        const uint32_t counts[] = {0, 1, 63, 64, 65, 2048};
        for (uint32_t want : counts)
            for (int variant = 0; variant < 3; ++variant) {
                std::vector<uint32_t> x(xn::LANES * xn::ELEMS), back;
                for (uint32_t& v : x) { const uint32_t r = rnd(); v = bookv[(r >> 23) % bookv.size()] << 23 | (r & 0x7fffffu); }
                std::vector<uint32_t> where;
                if (want == 2048) for (uint32_t i = 0; i < 2048; ++i) where.push_back(i);
                else {
                    std::vector<char> used(2048, 0);
                    if (want > 0 && variant == 1) { where.push_back(0); used[0] = 1; }
                    if (want > 1 && variant == 1) { where.push_back(2047); used[2047] = 1; }
                    if (want == 1 && variant == 2) { where.push_back(2047); used[2047] = 1; }
                    while (where.size() < want) { const uint32_t p = rnd() % 2048u; if (!used[p]) { used[p] = 1; where.push_back(p); } }
                }
                for (uint32_t p : where) { const uint32_t r = rnd(); x[p] = rarev[(r >> 23) % rarev.size()] << 23 | (r & 0x7fffffu); }
                const Record rec = encode_record(x, cls, 8);
                if (rec.neither || rec.entries.size() != want) return fail("exception count", want, rec.entries.size(), variant);
                for (size_t j = 1; j < rec.entries.size(); ++j)
                    if ((rec.entries[j] & 2047u) <= (rec.entries[j - 1] & 2047u)) return fail("entries are ordered by position", want, j, 0);
                decode_record(rec, books, back);
                for (size_t i = 0; i < x.size(); ++i)
                    if (back[i] != x[i]) return fail("record round trip", want, i, x[i]);
                ++checked;
            }
        // padding: rows past rows_valid hold anything at all in the lane's registers, give no entry and no report
        std::vector<uint32_t> x(xn::LANES * xn::ELEMS, 0xffc00000u), back;
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t i = 0; i < 12; ++i) x[lane * 32 + i] = rarev[(lane + i) % rarev.size()] << 23 | (rnd() & 0x7fffffu);
        const Record rec = encode_record(x, cls, 3);
        if (rec.neither || rec.entries.size() != 64 * 12) return fail("padding rows", rec.neither, rec.entries.size(), 0);
        decode_record(rec, books, back);
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t i = 0; i < 32; ++i) {
                if (i < 12 && back[lane * 32 + i] != x[lane * 32 + i]) return fail("rows before the padding", lane, i, 0);
                if (i >= 12 && (back[lane * 32 + i] >> 23) >= 255u) return fail("padding must decode to a finite positive number", lane, i, back[lane * 32 + i]);
            }
        if (encode_record(x, cls, 0).entries.size() != 0) return fail("a lane past the last column has no entries", 0, 0, 0);
    }

    // 3. the book from a histogram with ties: larger counts first, ties to the smaller value; the window alone supplies candidates
    {
        uint64_t hist[256] = {};
        hist[122] = hist[123] = hist[124] = hist[125] = hist[126] = hist[127] = hist[128] = hist[129] = 50;    // eight tied
        hist[0] = 50;                                                                                           // ... and zero
        hist[121] = 7; hist[120] = 7; hist[119] = 9;
        hist[3] = 1000000;                     // below the window of base 50 (top bytes 50..64: exponent bytes 100..129): no candidate
        xn::Books b;
        uint8_t cls[256];
        int nrare = 0;
        const uint64_t exc = xn::choose_books(hist, 50, b, cls, nrare);
        const uint32_t want_book[7] = {0, 122, 123, 124, 125, 126, 127};
        for (uint32_t i = 0; i < 7; ++i)
            if (xn::book_entry(b, i) != want_book[i] || cls[want_book[i]] != i) return fail("book with ties", i, xn::book_entry(b, i), want_book[i]);
        if (b.hi >> 24) return fail("byte 7 of the book is 0", b.hi, 0, 0);
        const uint32_t want_rare[5] = {128, 129, 119, 120, 121};
        for (uint32_t j = 0; j < 5; ++j)
            if (xn::rare_entry(b, j) != want_rare[j] || cls[want_rare[j]] != xn::CLS_RARE + j) return fail("rare book with ties", j, xn::rare_entry(b, j), want_rare[j]);
        if (exc != 50 + 50 + 9 + 7 + 7) return fail("exception count of the histogram", exc, 0, 0);
        if (nrare != 25 || cls[3] != xn::CLS_NONE) return fail("the window alone supplies candidates", nrare, cls[3], 0);
        for (uint32_t j = 0; j < 32; ++j) {          // rare_entry against the bytes of the table, every index
            const uint32_t direct = b.rare[j / 4] >> (8 * (j % 4)) & 0xffu;
            if (xn::rare_entry(b, j) != direct) return fail("rare_entry", j, xn::rare_entry(b, j), direct);
        }
    }

    // 4. directory offsets: a prefix sum; a grid whose entry count passes 2^32 is refused, one just below it is not
    {
        const uint32_t small[5] = {3, 0, 65, 2048, 1};
        uint32_t dir[6];
        if (!xn::build_directory(small, 5, dir)) return fail("small directory refused", 0, 0, 0);
        const uint32_t want[6] = {0, 3, 3, 68, 2116, 2117};
        for (int i = 0; i < 6; ++i)
            if (dir[i] != want[i]) return fail("directory", (unsigned)i, dir[i], want[i]);
        const uint64_t nrec = 2100000;                               // x 2048 entries = 4.3e9 > 2^32
        std::vector<uint32_t> counts(nrec, 2048u), big(nrec + 1);
        if (xn::build_directory(counts.data(), nrec, big.data())) return fail("a directory past 2^32 entries must be refused", 0, 0, 0);
        const uint64_t fit = xn::DIR_MAX / 2048u;
        if (!xn::build_directory(counts.data(), fit, big.data())) return fail("a directory below the limit refused", fit, 0, 0);
        if (big[fit] != (uint32_t)(fit * 2048u) || big[fit - 1] != (uint32_t)((fit - 1) * 2048u)) return fail("offsets near 2^32", big[fit], 0, 0);
        if ((uint64_t)big[fit] + 64u + 63u > 0xffffffffull) return fail("a wave's stride past the last entry must not wrap", big[fit], 0, 0);
        if (xn::build_directory(counts.data(), fit + 1, big.data())) return fail("a directory above the limit accepted", fit, 0, 0);
    }

    // 5. the fixed part: the dwords of the lanes tile the 6.5 KiB, every mantissa and code bit has one place in a lane's 26
    //    dwords, and records tile the copy
    {
        if (xn::RECORD_BYTES != 6656) return fail("a record is 6.5 KiB", xn::RECORD_BYTES, 0, 0);
        std::vector<int> hit(xn::RECORD_BYTES / 4, 0);
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t k = 0; k < xn::LANE_DWORDS; ++k) {
                const uint32_t off = xn::dword_offset(k, lane);
                if (off % 4 || off >= xn::RECORD_BYTES) return fail("dword offset", lane, k, off);
                hit[off / 4] += 1;
            }
        for (size_t i = 0; i < hit.size(); ++i)
            if (hit[i] != 1) return fail("record dword not covered exactly once", i, (unsigned)hit[i], 0);
        for (uint32_t lane = 0; lane < 64; ++lane)        // what the wave-wide loads assume: slot s at 1 KiB s + 16 lane, the last at 8 lane
            if (xn::dword_offset(4, lane) != 1024 + 16 * lane || xn::dword_offset(24, lane) != 6144 + 8 * lane) return fail("slot layout", lane, 0, 0);
        std::vector<int> bit(32 * xn::LANE_DWORDS, 0);
        for (uint32_t u = 0; u < 8; ++u)
            for (uint32_t e = 0; e < 4; ++e) {
                for (uint32_t j = 0; j < 23; ++j) bit[xn::mant_bit(u, e, j)] += 1;
                for (uint32_t j = 0; j < 3; ++j) bit[xn::code_bit(u, e, j)] += 1;
            }
        for (size_t i = 0; i < bit.size(); ++i)
            if (bit[i] != 1) return fail("lane bit not covered exactly once", i, (unsigned)bit[i], 0);
        std::vector<int> pos(8 * 72 * 8, 0);
        for (uint32_t p = 0; p < 2048; ++p) pos[xn::map_offset(p, 72 * 8)] += 1;
        for (uint32_t u = 0; u < 8; ++u)
            for (uint32_t b = 0; b < 72 * 8; ++b)
                if (pos[u * 72 * 8 + b] != (b < 256 ? 1 : 0)) return fail("the map is 256 bytes at the start of each tile row", u, b, 0);
        if (xn::record_offset(250000, 3999, 4000) != (250000ull * 4000ull + 3999ull) * 6656ull) return fail("64-bit record offset", 0, 0, 0);
        if (xn::record_index(1, 5, 12) != xn::record_index(1, 4, 12) + 1) return fail("panels of a chunk are adjacent", 0, 0, 0);
    }
    std::printf("ok %llu records, %llu with an element in neither book\n", checked, reported);
    return 0;
}
