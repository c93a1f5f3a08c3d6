// CPU model of the pre-tokeniser with digit groups: the GPT-2 flags from the per-position rules of
// yet-another-bpe_amd/csrc/pretok_logic.h, then the grouping of csrc/group_logic.h in the three steps the HIP kernels take
// (k_grp_windows / k_grp_carry / k_grp_apply): a state per 16-byte piece and per window of GRP_WIN bytes, the exclusive scan
// of the window states, then every piece walked behind its carry.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/group_logic.h"
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

// 1 iff special s begins with a \p{N} character (what yabpe_pretokenize rejects when G >= 1)
extern "C" int group_special_leads_with_digit(const uint8_t *bytes, uint32_t len) {
    build_table();
    const PtView v{bytes, nullptr, len, 0};
    uint32_t cp = 0;
    return pt_decode(v, 0, len, &cp) && g_cls[cp] == PT_N;
}

// The grouping alone, on meta / flags as the GPT-2 passes leave them (flags: 0, GRP_START, GRP_INSIDE) -> flags 0 / 1.
static void group_flags(const uint8_t *meta, uint8_t *flags, uint64_t n, uint32_t G) {
    const uint64_t n_win = (n + GRP_WIN - 1) / GRP_WIN, per_win = GRP_WIN / GRP_PIECE;
    auto piece = [&](uint64_t g) {
        return [=](int k, uint8_t *m, uint8_t *f) {
            *m = g + k < n ? meta[g + k] : (uint8_t)PT_O;
            *f = g + k < n ? flags[g + k] : (uint8_t)0;
        };
    };
    // step 1: the state of every window
    std::vector<GrpState> win(n_win, 0);
    for (uint64_t w = 0; w < n_win; ++w)
        for (uint64_t t = 0; t < per_win; ++t) win[w] = grp_combine(win[w], grp_piece_state(piece(w * GRP_WIN + t * GRP_PIECE), G), G);
    // step 2: exclusive scan, in place
    GrpState run = 0;
    for (uint64_t w = 0; w < n_win; ++w) {
        const GrpState mine = win[w];
        win[w] = run;
        run = grp_combine(run, mine, G);
    }
    // step 3: every window behind its carry; a piece's old flags are read before its new ones are written
    for (uint64_t w = 0; w < n_win; ++w) {
        GrpState before = win[w];
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * GRP_WIN + t * GRP_PIECE;
            const GrpState mine = grp_piece_state(piece(g), G);
            uint8_t out[GRP_PIECE];
            grp_piece_flags(before, piece(g), [&](int k, uint8_t f) { out[k] = f; }, G);
            for (int k = 0; k < GRP_PIECE && g + k < n; ++k) flags[g + k] = out[k];
            before = grp_combine(before, mine, G);
        }
    }
}

// flags_out[i] = 1 iff a pre-token of the grouped pattern starts at byte i (G = 0: of the GPT-2 pattern).  *err_pos = first
// malformed byte (UnicodeDecodeError.start) or -1.
extern "C" int group_model(const uint8_t *text, uint64_t n, const uint64_t *chunk_off, uint32_t n_chunks, const uint8_t *sp_bytes,
                           const uint32_t *sp_off, uint32_t n_sp, uint32_t G, uint8_t *flags_out, int64_t *err_pos) {
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
        meta[i] = (uint8_t)((meta[i] & PT_CHUNK0) | m);
        if (bad && *err_pos < 0) *err_pos = (int64_t)i;
    }
    if (*err_pos >= 0) return 0;
    PtView v{text, meta.data(), n, 0};
    for (uint64_t i = 0; i < n; ++i) flags_out[i] = pt_is_start(v, i, -1) ? 1 : 0;
    if (n_sp) {
        uint32_t max_len = 0;
        for (uint32_t s = 0; s < n_sp; ++s) max_len = sp_off[s + 1] - sp_off[s] > max_len ? sp_off[s + 1] - sp_off[s] : max_len;
        PtSpecials sp{sp_bytes, sp_off, n_sp, max_len};
        auto occ = [&](uint64_t q) -> uint32_t { return pt_special_at(v, sp, q); };
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t o = occ(i);
            if (o && pt_special_is_head(v, sp, occ, i)) pt_special_walk(v, sp, occ, flags_out, i, o, (uint8_t)(G ? GRP_INSIDE : 0));
        }
    }
    if (G && n) group_flags(meta.data(), flags_out, n, G);
    return 0;
}
