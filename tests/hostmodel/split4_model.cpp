// CPU model of the pre-tokeniser with the cl100k pattern: the per-position rules of yet-another-bpe_amd/csrc/split4_logic.h
// (pt4_is_start, the special chains), then the newline pass in the three steps the HIP kernels take (k_nl_windows /
// k_nl_carry / k_nl_apply: a state per 16-byte piece and per window, the carry in tiles of 2,048 windows in both directions,
// every piece resolved between its carries), then the digit groups of csrc/group_logic.h.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/split4_logic.h"
#include "../../yet-another-bpe_amd/csrc/unicode_classes.inc"

static std::vector<uint8_t> g_cls;

static void build_table() {
    if (!g_cls.empty()) return;
    g_cls.assign(0x110000, PT_O);
    for (unsigned r = 0; r < YB_UNICODE_CLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_CLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_CLASS_NRUNS ? YB_UNICODE_CLASS_RUNS[r + 1][0] : 0x110000;
        memset(g_cls.data() + lo, (int)YB_UNICODE_CLASS_RUNS[r][1], hi - lo);
    }
}

// class of the first character of a special (PT_L .. PT_O), -1 when it does not decode: what yabpe_pretokenize looks at
extern "C" int split4_special_lead_class(const uint8_t *bytes, uint32_t len) {
    build_table();
    const PtView v{bytes, nullptr, len, 0};
    uint32_t cp = 0;
    return pt_decode(v, 0, len, &cp) ? (int)g_cls[cp] : -1;
}

// The 16-bytes-at-once masks of nl_piece against the per-byte definitions, for every meta / flag value a byte can have, at
// every place in a piece.  0 when they agree.
extern "C" int split4_masks_selfcheck() {
    for (uint32_t meta = 0; meta < 32; ++meta)
        for (uint32_t flag = 0; flag <= PT4_PENDING; ++flag)
            for (int k = 0; k < GRP_PIECE; ++k) {
                uint32_t m[4] = {0, 0, 0, 0}, f[4] = {0, 0, 0, 0};
                for (int j = 0; j < GRP_PIECE; ++j) m[j >> 2] |= (uint32_t)(PT_CONT | PT_L) << ((j & 3) * 8); // "keep" in both senses
                m[k >> 2] = (m[k >> 2] & ~(0xFFu << ((k & 3) * 8))) | (meta << ((k & 3) * 8));
                f[k >> 2] = flag << ((k & 3) * 8);
                const NlPiece p = nl_piece(m, f);
                const uint32_t ef = nl_fwd_byte((uint8_t)meta, (uint8_t)flag), eb = nl_bwd_byte((uint8_t)meta, (uint8_t)flag);
                if (nl_piece_state(p) != (ef | (eb << NL_BWD))) return 1;
                if (p.pending != (flag == PT4_PENDING ? 1u << k : 0u)) return 2;
            }
    return 0;
}

static const uint64_t TILE = 256 * 8; // windows per iteration of k_nl_carry

static void newline_flags(const uint8_t *meta, uint8_t *flags, uint64_t n) {
    const uint64_t n_win = (n + GRP_WIN - 1) / GRP_WIN, per_win = GRP_WIN / GRP_PIECE;
    struct Words {
        uint32_t m[4], f[4];
    };
    auto words = [&](uint64_t g) { // as grp_load of the kernels
        Words p{};
        for (int k = 0; k < GRP_PIECE; ++k) {
            p.m[k >> 2] |= (uint32_t)(g + k < n ? meta[g + k] : (uint8_t)PT_O) << ((k & 3) * 8);
            p.f[k >> 2] |= (uint32_t)(g + k < n ? flags[g + k] : (uint8_t)0) << ((k & 3) * 8);
        }
        return p;
    };
    auto piece = [&](uint64_t g) {
        const Words p = words(g);
        return nl_piece(p.m, p.f);
    };
    auto fwd = [](NlState s) { return s & NL_MASK; };
    auto bwd = [](NlState s) { return (s >> NL_BWD) & NL_MASK; };
    // step 1: both summaries of every window
    std::vector<NlState> win(n_win, 0);
    for (uint64_t w = 0; w < n_win; ++w) {
        uint32_t f = NL_KEEP, b = NL_KEEP;
        for (uint64_t t = 0; t < per_win; ++t) f = nl_comb(f, fwd(nl_piece_state(piece(w * GRP_WIN + t * GRP_PIECE))));
        for (uint64_t t = per_win; t-- > 0;) b = nl_comb(b, bwd(nl_piece_state(piece(w * GRP_WIN + t * GRP_PIECE))));
        win[w] = f | (b << NL_BWD);
    }
    // step 2: in place, tile by tile with a carry: forward left to right, backward right to left
    const uint64_t n_tiles = (n_win + TILE - 1) / TILE;
    uint32_t carry = NL_KEEP;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint32_t run = carry;
        for (uint64_t w = t * TILE; w < std::min(n_win, (t + 1) * TILE); ++w) {
            const uint32_t mine = fwd(win[w]);
            win[w] = (win[w] & ~NL_MASK) | run;
            run = nl_comb(run, mine);
        }
        carry = run;
    }
    carry = NL_KEEP;
    for (uint64_t t = n_tiles; t-- > 0;) {
        uint32_t run = carry;
        for (uint64_t w = std::min(n_win, (t + 1) * TILE); w-- > t * TILE;) {
            const uint32_t mine = bwd(win[w]);
            win[w] = (win[w] & NL_MASK) | (run << NL_BWD);
            run = nl_comb(run, mine);
        }
        carry = run;
    }
    // step 3: every window between its carries; a piece's old flags are read before its new ones are written
    std::vector<uint32_t> after(per_win);
    for (uint64_t w = 0; w < n_win; ++w) {
        uint32_t b = bwd(win[w]);
        for (uint64_t t = per_win; t-- > 0;) {
            after[t] = b;
            b = nl_comb(b, bwd(nl_piece_state(piece(w * GRP_WIN + t * GRP_PIECE))));
        }
        uint32_t before = fwd(win[w]);
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * GRP_WIN + t * GRP_PIECE;
            const uint32_t mine = fwd(nl_piece_state(piece(g)));
            Words p = words(g);
            nl_piece_flags(before, after[t], nl_piece(p.m, p.f), p.f);
            for (int k = 0; k < GRP_PIECE && g + k < n; ++k) flags[g + k] = (uint8_t)(p.f[k >> 2] >> ((k & 3) * 8));
            before = nl_comb(before, mine);
        }
    }
}

static void group_flags(const uint8_t *meta, uint8_t *flags, uint64_t n, uint32_t G) {
    const uint64_t n_win = (n + GRP_WIN - 1) / GRP_WIN, per_win = GRP_WIN / GRP_PIECE;
    auto piece = [&](uint64_t g) {
        return [=](int k, uint8_t *m, uint8_t *f) {
            *m = g + k < n ? meta[g + k] : (uint8_t)PT_O;
            *f = g + k < n ? flags[g + k] : (uint8_t)0;
        };
    };
    GrpState before = 0;
    for (uint64_t w = 0; w < n_win; ++w)
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * GRP_WIN + t * GRP_PIECE;
            const GrpState mine = grp_piece_state(piece(g), G);
            uint8_t out[GRP_PIECE];
            grp_piece_flags(before, piece(g), [&](int k, uint8_t f) { out[k] = f; }, G);
            for (int k = 0; k < GRP_PIECE && g + k < n; ++k) flags[g + k] = out[k];
            before = grp_combine(before, mine, G);
        }
}

// flags_out[i] = 1 iff a pre-token of the cl100k pattern with \p{N}{1,G} starts at byte i.  *err_pos = first malformed byte
// (UnicodeDecodeError.start) or -1.  stage: 0 everything; 1 stop behind the local and special passes (flags 0 .. 4).
extern "C" int split4_model(const uint8_t *text, uint64_t n, const uint64_t *chunk_off, uint32_t n_chunks, const uint8_t *sp_bytes,
                            const uint32_t *sp_off, uint32_t n_sp, uint32_t G, uint32_t stage, uint8_t *flags_out, int64_t *err_pos) {
    build_table();
    std::vector<uint8_t> meta(n, 0);
    for (uint32_t c = 0; c < n_chunks; ++c)
        if (chunk_off[c] < n) meta[chunk_off[c]] |= PT_CHUNK0;
    *err_pos = -1;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t end = n;
        for (uint64_t k = i + 1; k < i + 4 && k < n; ++k)
            if (meta[k] & PT_CHUNK0) {
                end = k;
                break;
            }
        bool bad = false;
        const PtView v0{text, meta.data(), n, 0};
        const uint8_t m = pt_classify(v0, i, end, g_cls.data(), &bad);
        meta[i] = (uint8_t)((meta[i] & PT_CHUNK0) | m | (pt4_is_nl(text[i]) ? PT4_NL : 0));
        if (bad && *err_pos < 0) *err_pos = (int64_t)i;
    }
    if (*err_pos >= 0) return 0;
    PtView v{text, meta.data(), n, 0};
    for (uint64_t i = 0; i < n; ++i) flags_out[i] = pt4_is_start(v, i, -1);
    if (n_sp) {
        uint32_t max_len = 0;
        for (uint32_t s = 0; s < n_sp; ++s) max_len = std::max(max_len, sp_off[s + 1] - sp_off[s]);
        PtSpecials sp{sp_bytes, sp_off, n_sp, max_len};
        auto occ = [&](uint64_t q) -> uint32_t { return pt_special_at(v, sp, q); };
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t o = occ(i);
            if (o && pt4_special_is_head(v, sp, occ, i)) pt4_special_walk(v, sp, occ, flags_out, i, o);
        }
    }
    if (stage == 1 || n == 0) return 0;
    newline_flags(meta.data(), flags_out, n);
    group_flags(meta.data(), flags_out, n, G);
    return 0;
}
