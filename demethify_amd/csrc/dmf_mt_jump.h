// Jump-ahead for MT19937 (dmf_mt_jump.hip, host only): the polynomial that carries a key a whole number of 624-word
// blocks forward, as the list of its non-zero terms.  See the head of dmf_mt_jump.hip.
#pragma once
#include <cstdint>
#include <vector>

namespace dmf {

constexpr int kMtJumpDegree = 19937;  // of the characteristic polynomial phi
// the raw words a jump reads behind a key's first: x[i + m] for a term i <= 19937 and a result word m < 624, held as
// whole blocks -- the key and 32 regenerations of it
constexpr int kMtJumpBlocks = 33, kMtJumpWords = kMtJumpBlocks * 624;

// g = t^(624 blocks) mod (t phi) as the ascending list of the exponents of its non-zero terms (each <= 19937).  Computed at
// first use, kept for the life of the process (the reference stays valid), thread-safe.
const std::vector<uint16_t>& mt_jump_terms(uint64_t blocks);

// key <- the key `blocks` regenerations later (blocks >= 1), by the polynomial; word 0's low 31 bits are never read.
void mt_jump_key(uint32_t key[624], uint64_t blocks);

}  // namespace dmf
