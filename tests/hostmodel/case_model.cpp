// CPU model of yabpe_lowercase: the rules of yet-another-bpe_amd/csrc/case_logic.h (the functions the HIP kernels call) run
// piece by piece and window by window over a text cut into parts, with the part starts as marks.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/case_logic.h"
#include "../../yet-another-bpe_amd/csrc/unicode_case.inc"

static std::vector<uint32_t> g_tab;

static const uint32_t *table() {
    if (g_tab.empty()) {
        g_tab.resize(CASE_NCP);
        if (!case_expand(g_tab.data(), YB_CASE_LOWER, YB_CASE_NLOWER, YB_CASE_TWO, YB_CASE_CASED, YB_CASE_NCASED, YB_CASE_IGNORABLE, YB_CASE_NIGNORABLE))
            g_tab.assign(CASE_NCP, 0xFFFFFFFFu);
    }
    return g_tab.data();
}

extern "C" const char *case_model_version() { return YB_CASE_UNIDATA_VERSION; }

// (piece, window, carry tile in windows) as the headers name them
extern "C" void case_model_sizes(uint32_t *out) {
    out[0] = CASE_PIECE;
    out[1] = CASE_WIN;
}

// the expanded table: CASE_NCP entries (lowered code point | cased << 21 | ignorable << 22 | two << 23)
extern "C" void case_model_table(uint32_t *out) { memcpy(out, table(), CASE_NCP * 4); }

extern "C" uint32_t case_model_ascii_state(uint32_t b) { return case_ascii_state(b); }
extern "C" uint32_t case_model_upper_bits4(uint32_t w) { return case_upper_bits4(w); }

// Exclusive scan of the piece states as the three launches do it: per window, the carry over the windows, then inside.
static void scan_states(const std::vector<uint32_t> &st, bool fwd, std::vector<uint32_t> *ex) {
    const size_t np = st.size(), ppw = CASE_WIN / CASE_PIECE, nw = (np + ppw - 1) / ppw;
    std::vector<uint32_t> win(nw, CASE_ST_NONE), carry(nw, CASE_ST_NONE);
    for (size_t w = 0; w < nw; ++w) {
        uint32_t t = CASE_ST_NONE;
        for (size_t j = 0; j < ppw; ++j) {
            const size_t p = w * ppw + (fwd ? j : ppw - 1 - j);
            if (p < np) t = case_combine(t, st[p]);
        }
        win[w] = t;
    }
    uint32_t run = CASE_ST_NONE;
    for (size_t i = 0; i < nw; ++i) {
        const size_t w = fwd ? i : nw - 1 - i;
        carry[w] = run;
        run = case_combine(run, win[w]);
    }
    ex->assign(np, CASE_ST_NONE);
    for (size_t w = 0; w < nw; ++w) {
        uint32_t t = carry[w];
        for (size_t j = 0; j < ppw; ++j) {
            const size_t p = w * ppw + (fwd ? j : ppw - 1 - j);
            if (p >= np) continue;
            (*ex)[p] = t;
            t = case_combine(t, st[p]);
        }
    }
}

// Returns 0 (text in out[0..*out_n), part offsets in out_off[0..n_parts]), -7 for malformed UTF-8 (counts[0] = the position),
// -8 when cap is too small, -5 when two passes disagree.  counts = (first malformed byte or ~0, code points that change, length
// changers, sigmas, final sigmas, path).  part_off: n_parts ascending starts, the first one 0.
extern "C" int case_model(const uint8_t *text, uint64_t n, const uint64_t *part_off, uint32_t n_parts, uint8_t *out, uint64_t cap, uint64_t *out_n,
                          uint64_t *out_off, uint64_t *counts) {
    const CaseTables T{table()};
    std::vector<uint8_t> mark(n + 1, 0);
    for (uint32_t k = 0; k < n_parts; ++k)
        if (part_off[k] < n) mark[part_off[k]] = PT_CHUNK0;
    const PtView v{text, n_parts == 1 ? nullptr : mark.data(), n, 0};  // (one part: no marks, as the driver calls the kernels)
    const uint64_t n_pieces = (n + CASE_PIECE - 1) / CASE_PIECE, n_win = (n + CASE_WIN - 1) / CASE_WIN;
    // check
    CaseCounts all{~0ull, 0, 0, 0, 0};
    std::vector<uint64_t> wout(n_win + 1, 0);
    for (uint64_t p = 0; p < n_pieces; ++p) {
        CaseCounts c{~0ull, 0, 0, 0, 0};
        case_check_piece(v, T, p * CASE_PIECE, &c);
        all.bad = c.bad < all.bad ? c.bad : all.bad;
        all.changed += c.changed;
        all.resized += c.resized;
        all.sigma += c.sigma;
        wout[p * CASE_PIECE / CASE_WIN] += c.out;
    }
    counts[0] = all.bad; counts[1] = all.changed; counts[2] = all.resized; counts[3] = all.sigma; counts[4] = 0; counts[5] = 0;
    if (all.bad != ~0ull) return -7;
    auto input_offsets = [&]() {
        for (uint32_t k = 0; k < n_parts; ++k) out_off[k] = part_off[k];
        out_off[n_parts] = n;
        *out_n = n;
    };
    if (n > cap) return -8;
    if (all.changed == 0) {
        memcpy(out, text, n);
        input_offsets();
        return 0;
    }
    if (all.resized == 0 && all.sigma == 0) {
        counts[5] = 1;
        for (uint64_t p = 0; p < n_pieces; ++p) {
            uint64_t lo, hi;
            case_same_piece(v, T, p * CASE_PIECE, &lo, &hi);
            for (uint64_t k = 0; k < CASE_PIECE && p * CASE_PIECE + k < n; ++k) out[p * CASE_PIECE + k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu);
        }
        input_offsets();
        return 0;
    }
    counts[5] = 2;
    // final sigmas
    std::vector<uint32_t> fin(n_pieces, 0);
    if (all.sigma) {
        std::vector<uint32_t> st(n_pieces), ex;
        for (uint64_t p = 0; p < n_pieces; ++p) st[p] = case_piece_fwd(v, T, p * CASE_PIECE);
        scan_states(st, true, &ex);
        for (uint64_t p = 0; p < n_pieces; ++p) fin[p] = case_piece_mark_fwd(v, T, p * CASE_PIECE, ex[p]);
        for (uint64_t p = 0; p < n_pieces; ++p) st[p] = case_piece_bwd(v, T, p * CASE_PIECE);
        scan_states(st, false, &ex);
        for (uint64_t p = 0; p < n_pieces; ++p) {
            fin[p] = case_piece_mark_bwd(v, T, p * CASE_PIECE, ex[p], fin[p]);
            counts[4] += (uint64_t)__builtin_popcount(fin[p]);
        }
    }
    // write: every window starts where the scan of the window sizes says
    uint64_t o = 0, base = 0;
    uint32_t k = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % CASE_WIN == 0) {
            if (o != base) return -5;
            base += wout[i / CASE_WIN];
        }
        while (k < n_parts && part_off[k] == i) out_off[k++] = o;
        const uint32_t ol = case_byte_out_len(v, T, i);
        if (ol == 0) continue;
        if (o + 4 > cap) return -8;
        uint32_t len = 0;
        case_emit(v, T, i, (fin[i / CASE_PIECE] >> (i % CASE_PIECE)) & 1u, out + o, &len);
        if (len != ol) return -5;
        o += len;
    }
    if (o != base) return -5;
    while (k < n_parts) out_off[k++] = o;
    out_off[n_parts] = o;
    *out_n = o;
    return 0;
}
