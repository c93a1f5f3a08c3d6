// CPU model of yabpe_utf8_repair: the per-byte rules of yet-another-bpe_amd/csrc/utf8_logic.h (the functions the HIP kernels
// call) run sequentially over a text cut into parts, with the part starts as marks.  Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/utf8_logic.h"

// (piece, tile, halo) as the header names them
extern "C" void utf8_model_sizes(uint32_t *out) {
    out[0] = U8_PIECE;
    out[1] = U8_TILE;
    out[2] = U8_HALO;
}

static int run(const uint8_t *text, uint64_t n, const std::vector<uint8_t> &mark, uint64_t pos0, uint32_t mode, uint8_t *out, uint64_t cap, uint64_t *o,
               uint64_t *counts) {
    const U8View v{text, mark.data(), 0};
    uint32_t run = 1;
    for (uint64_t p = 0; p < n; ++p) {
        const uint32_t raw = u8_raw_len(v, p, n, true, &run), ol = u8_charge(raw, mode);
        if (*o + ol > cap) return -8;
        dec_emit(text[p], ol, out + *o);
        *o += ol;
        if (raw == 3) {
            if (counts[0]++ == 0) counts[1] = pos0 + p;
        }
    }
    return 0;
}

// Returns 0 (text in out[0..*out_n), part offsets in out_off[0..n_parts]), -8 when cap is too small, -1 for another mode.
// counts = (subparts replaced or dropped, position of the first one; ~0: none).  part_off: n_parts ascending starts, the first
// one 0.  isolated: every part is run as a text of its own (no marks, no neighbours) instead of as a part of the text.
extern "C" int utf8_model(const uint8_t *text, uint64_t n, const uint64_t *part_off, uint32_t n_parts, uint32_t mode, int isolated, uint8_t *out,
                          uint64_t cap, uint64_t *out_n, uint64_t *out_off, uint64_t *counts) {
    if (mode != U8_REPLACE && mode != U8_IGNORE) return -1;
    counts[0] = 0;
    counts[1] = ~0ull;
    uint64_t o = 0;
    if (isolated) {
        std::vector<uint8_t> part, mark;
        for (uint32_t k = 0; k < n_parts; ++k) {
            const uint64_t a = part_off[k], b = k + 1 < n_parts ? part_off[k + 1] : n;
            out_off[k] = o;
            part.assign(text + a, text + b);
            mark.assign(b - a + 1, 0);
            const int rc = run(part.data(), b - a, mark, a, mode, out, cap, &o, counts);
            if (rc) return rc;
        }
    } else {
        std::vector<uint8_t> mark(n + 1, 0);
        for (uint32_t k = 0; k < n_parts; ++k) mark[part_off[k]] = 1;
        const U8View v{text, mark.data(), 0};
        uint32_t k = 0;
        // as the kernels walk a piece: the bytes a well-formed lead settles are copied without asking again, up to the piece's end
        uint32_t run = 1, settled = 0;
        for (uint64_t p = 0; p < n; ++p) {
            while (k < n_parts && part_off[k] == p) out_off[k++] = o;
            if (p % U8_PIECE == 0) settled = 0;
            uint32_t raw = 1;
            if (settled) --settled;
            else if ((raw = u8_raw_len(v, p, n, true, &run)) == 1) settled = run - 1;
            const uint32_t ol = u8_charge(raw, mode);
            if (o + ol > cap) return -8;
            dec_emit(text[p], ol, out + o);
            o += ol;
            if (raw == 3) {
                if (counts[0]++ == 0) counts[1] = p;
            }
        }
        while (k < n_parts) out_off[k++] = o;
    }
    out_off[n_parts] = o;
    *out_n = o;
    return 0;
}
