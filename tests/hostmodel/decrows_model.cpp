// CPU model of the character-start rule of yet-another-bpe_amd/csrc/decode_logic.h (dec_char_start, the function k_drow_chars
// calls): out[p] = 1 when byte p of its document starts a character.  n_docs documents of len bytes each.  Test infrastructure only.
#include <stdint.h>

#include "../../yet-another-bpe_amd/csrc/decode_logic.h"

extern "C" void char_starts(const uint8_t *data, uint64_t n_docs, uint64_t len, uint8_t *out) {
    for (uint64_t d = 0; d < n_docs; ++d) {
        const DecView v{data + d * len, 0};
        for (uint64_t p = 0; p < len; ++p) out[d * len + p] = dec_char_start(v, p, 0, len) ? 1 : 0;
    }
}
