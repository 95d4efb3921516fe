// Jump-ahead for numpy's legacy generator (MT19937), host side: no device code and no HIP call in this file.
//
// Let x[0..623] be a key and x[i + 624] = x[i + 397] ^ tw(x[i], x[i + 1]) the raw (untempered) words that follow it.  From
// x[1] on, every bit of that sequence obeys the linear recurrence whose characteristic polynomial is phi(t), of degree
// 19937: sum_k phi_k x[j + k] = 0 for j >= 1.  The low 31 bits of x[0] are output but are not part of the 19937-bit state (a
// key set with np.random.set_state may hold anything there), so the sequence from x[0] on is annihilated by t phi(t) only.
// With g = t^J mod (t phi),  x[J + m] = XOR over { i : g_i = 1 } of x[i + m]  for every m >= 0 and all 32 bits: for J >= 1 the
// remainder is divisible by t and never reads x[0].  The key J words later is the 624 words m = 0..623.
//
// phi is not a table: it is found at first use by Berlekamp-Massey over GF(2) on the low bit of 2 * 19937 + 100 raw words of
// a seeded key (bit-packed, 64 sequence bits to a word), and its degree is asserted.  It has few terms, so the reduction of
// a square modulo t phi is a handful of shifted XORs per 64 bits, and t^J is square-and-multiply-by-t over the bits of J.
#include "dmf_mt_jump.h"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/demethify_hip.h"

namespace dmf {

namespace {

constexpr int kN = 624, kM = 397, kTop = kMtJumpDegree + 1;  // kTop: the degree of t phi
constexpr int kPolyWords = (kTop + 63) / 64;                  // a remainder: degree < kTop
using Poly = std::array<uint64_t, kPolyWords>;

inline uint32_t twist(uint32_t a, uint32_t b) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// n[0..623] <- the regeneration of o[0..623]
void regenerate(const uint32_t* o, uint32_t* n) {
    for (int i = 0; i < kN - kM; ++i) n[i] = o[i + kM] ^ twist(o[i], o[i + 1]);
    for (int i = kN - kM; i < kN - 1; ++i) n[i] = n[i - (kN - kM)] ^ twist(o[i], o[i + 1]);
    n[kN - 1] = n[kM - 1] ^ twist(o[kN - 1], n[0]);
}

[[noreturn]] void die(const char* what) {
    std::fprintf(stderr, "dmf_mt_jump: %s\n", what);
    std::abort();
}

// 64 bits of a bit-packed array from bit `at` on (the array is padded by a word)
inline uint64_t window(const uint64_t* a, size_t at) {
    const size_t w = at >> 6, b = at & 63;
    return b ? (a[w] >> b) | (a[w + 1] << (64 - b)) : a[w];
}

// The exponents below kTop of t phi(t), ascending, and kTop minus the largest of them.
struct Modulus {
    std::vector<int> low;
    int gap = 0;
};

Modulus find_modulus() {
    constexpr int kBits = 2 * kMtJumpDegree + 100, kWords = kBits / 64 + 3;
    // the low bit of the raw words from the first regeneration of a seeded key on, stored in reverse (bit k = s[kBits - 1 - k])
    // so that the window s[n], s[n - 1], ... of a discrepancy is an ascending run of bits
    std::vector<uint32_t> x((kBits / kN + 2) * kN);
    x[0] = 5489u;
    for (int i = 1; i < kN; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
    for (size_t b = 0; b + 2 * kN <= x.size(); b += kN) regenerate(&x[b], &x[b + kN]);
    const uint32_t* s = &x[kN];
    std::vector<uint64_t> rs(kWords, 0), C(kWords, 0), B(kWords, 0), T(kWords, 0);
    for (int n = 0; n < kBits; ++n)
        if (s[n] & 1u) rs[(kBits - 1 - n) >> 6] |= 1ull << ((kBits - 1 - n) & 63);
    C[0] = B[0] = 1;
    int L = 0, m = 1, degB = 0;
    for (int n = 0; n < kBits; ++n) {
        uint64_t acc = 0;  // the discrepancy: sum over i <= L of C_i s[n - i]
        const size_t at = (size_t)(kBits - 1 - n);
        for (int j = 0; j <= L >> 6; ++j) acc ^= C[j] & window(rs.data(), at + 64 * (size_t)j);
        if (!(__builtin_popcountll(acc) & 1)) {
            ++m;
            continue;
        }
        const bool longer = 2 * L <= n;
        if (longer) T = C;
        const int ws = m >> 6, bs = m & 63;  // C ^= B << m
        for (int j = 0; j <= degB >> 6; ++j) {
            C[j + ws] ^= B[j] << bs;
            if (bs) C[j + ws + 1] ^= B[j] >> (64 - bs);
        }
        if (longer) {
            const int degT = L;
            L = n + 1 - L;
            B.swap(T);
            degB = degT;
            m = 1;
        } else {
            ++m;
        }
    }
    if (L != kMtJumpDegree) die("the characteristic polynomial of MT19937 does not have degree 19937");
    // sum_i C_i s[n - i] = 0: phi_k = C_{L - k}, and t phi has the exponents k + 1
    Modulus mod;
    for (int k = 0; k < L; ++k)
        if (C[(L - k) >> 6] >> ((L - k) & 63) & 1) mod.low.push_back(k + 1);
    if (!(C[0] & 1) || mod.low.empty() || mod.low.front() != 1) die("the characteristic polynomial of MT19937 is malformed");
    mod.gap = kTop - mod.low.back();
    // every bit of the words behind the first obeys it (phi from x[1] on)
    for (int j = 1; j < 40; ++j) {
        uint32_t v = x[j + kMtJumpDegree];
        for (int e : mod.low) v ^= x[j + e - 1];
        if (v != 0) die("the characteristic polynomial of MT19937 does not annihilate the raw words");
    }
    return mod;
}

const Modulus& modulus() {
    static const Modulus mod = find_modulus();  // (thread-safe: a function-local static)
    return mod;
}

// a[0 .. words) of degree < 64 words, reduced below kTop modulo t phi, a chunk of at most 64 bits (and at most the gap, so
// that a chunk's image lies wholly below it) at a time from the top
void reduce(uint64_t* a, int words, const Modulus& mod) {
    const int chunk = mod.gap < 64 ? mod.gap : 64;
    for (int hi = 64 * words; hi > kTop;) {
        const int cw = hi - kTop < chunk ? hi - kTop : chunk, lo = hi - cw;
        const int w = lo >> 6, b = lo & 63;
        uint64_t v = a[w] >> b;
        if (b && w + 1 < words) v |= a[w + 1] << (64 - b);
        if (cw < 64) v &= (1ull << cw) - 1;
        if (v) {
            a[w] ^= v << b;
            if (b && w + 1 < words) a[w + 1] ^= v >> (64 - b);
            for (int e : mod.low) {
                const int at = lo - kTop + e, tw = at >> 6, tb = at & 63;
                a[tw] ^= v << tb;
                if (tb) a[tw + 1] ^= v >> (64 - tb);  // (at + cw <= lo: inside the array)
            }
        }
        hi = lo;
    }
}

inline uint64_t spread(uint32_t v) {  // bit i -> bit 2 i
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// t^J mod (t phi)
Poly power_of_t(unsigned __int128 J) {
    const Modulus& mod = modulus();
    Poly r{};
    r[0] = 1;
    int top = 127;
    while (top >= 0 && !(J >> top & 1)) --top;
    std::array<uint64_t, 2 * kPolyWords + 1> sq;
    for (int bit = top; bit >= 0; --bit) {
        for (int j = 0; j < kPolyWords; ++j) {
            sq[2 * j] = spread((uint32_t)r[j]);
            sq[2 * j + 1] = spread((uint32_t)(r[j] >> 32));
        }
        sq[2 * kPolyWords] = 0;
        reduce(sq.data(), 2 * kPolyWords, mod);
        std::memcpy(r.data(), sq.data(), sizeof(Poly));
        if (J >> bit & 1) {  // times t
            uint64_t carry = 0;
            for (int j = 0; j < kPolyWords; ++j) {
                const uint64_t next = r[j] >> 63;
                r[j] = (r[j] << 1) | carry;
                carry = next;
            }
            if (r[kTop >> 6] >> (kTop & 63) & 1) {
                r[kTop >> 6] ^= 1ull << (kTop & 63);
                for (int e : mod.low) r[e >> 6] ^= 1ull << (e & 63);
            }
        }
    }
    return r;
}

std::mutex g_cache_mutex;
std::map<uint64_t, std::vector<uint16_t>> g_cache;  // by the number of blocks (a node's vector never moves)

}  // namespace

const std::vector<uint16_t>& mt_jump_terms(uint64_t blocks) {
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    auto it = g_cache.find(blocks);
    if (it != g_cache.end()) return it->second;
    const Poly g = power_of_t((unsigned __int128)blocks * kN);
    std::vector<uint16_t> terms;
    for (int i = 0; i < kTop; ++i)
        if (g[i >> 6] >> (i & 63) & 1) terms.push_back((uint16_t)i);
    return g_cache.emplace(blocks, std::move(terms)).first->second;
}

void mt_jump_key(uint32_t key[624], uint64_t blocks) {
    const std::vector<uint16_t>& terms = mt_jump_terms(blocks);
    std::vector<uint32_t> x(kMtJumpWords);
    std::memcpy(x.data(), key, kN * sizeof(uint32_t));
    for (int b = 0; b + 1 < kMtJumpBlocks; ++b) regenerate(&x[b * kN], &x[(b + 1) * kN]);
    uint32_t out[kN] = {};
    for (uint16_t i : terms) {
        const uint32_t* w = &x[i];
        for (int m = 0; m < kN; ++m) out[m] ^= w[m];
    }
    std::memcpy(key, out, sizeof(out));
}

}  // namespace dmf

extern "C" int dmf_mt_jump(uint32_t key[624], int* pos, uint64_t n_words) {
    if (key == nullptr || pos == nullptr || *pos < 0 || *pos > 624) return DMF_ERR_BAD_ARG;
    if (n_words == 0) return DMF_OK;
    // x[0..623] the key: the words used are x[pos .. pos + n_words); numpy holds the key of the block with the last of them
    const unsigned __int128 last = (unsigned __int128)(unsigned)*pos + n_words - 1;
    const uint64_t block = (uint64_t)(last / 624);
    if (block > 0) dmf::mt_jump_key(key, block);
    *pos = (int)(uint64_t)(last - (unsigned __int128)block * 624) + 1;
    return DMF_OK;
}
