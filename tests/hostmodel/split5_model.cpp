// CPU model of the pre-tokeniser with the o200k_base pattern: the functions of yet-another-bpe_amd/csrc/split5_logic.h in the
// steps the HIP kernels take -- classes (k_s5_class), the look-ahead scan backward (k_la_windows / k_la_carry / k_la_apply: a
// value per 16-byte piece and per window, the carry in tiles of 2,048 windows), the aux bytes and the special marks (k_s5_aux,
// k_s5_special), the function scan forward (k_fn_windows / k_fn_carry / k_fn_apply, same geometry), then the digit groups of
// csrc/group_logic.h.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/split5_logic.h"
#include "../../yet-another-bpe_amd/csrc/unicode_classes.inc"
#include "../../yet-another-bpe_amd/csrc/unicode_subclasses.inc"

static std::vector<uint8_t> g_cls;

static void build_table() {
    if (!g_cls.empty()) return;
    std::vector<uint8_t> cls(0x110000, PT_O), sub(0x110000, 0);
    for (unsigned r = 0; r < YB_UNICODE_CLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_CLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_CLASS_NRUNS ? YB_UNICODE_CLASS_RUNS[r + 1][0] : 0x110000;
        memset(cls.data() + lo, (int)YB_UNICODE_CLASS_RUNS[r][1], hi - lo);
    }
    for (unsigned r = 0; r < YB_UNICODE_SUBCLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_SUBCLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_SUBCLASS_NRUNS ? YB_UNICODE_SUBCLASS_RUNS[r + 1][0] : 0x110000;
        memset(sub.data() + lo, (int)YB_UNICODE_SUBCLASS_RUNS[r][1], hi - lo);
    }
    g_cls.resize(0x110000);
    for (uint32_t cp = 0; cp < 0x110000; ++cp) g_cls[cp] = pt5_table_entry(cp, cls[cp], sub[cp]);
}

// the scanner's class (C5_U .. C5_O) of every code point, into out[0x110000]
extern "C" void split5_classes(uint8_t *out) {
    build_table();
    for (uint32_t cp = 0; cp < 0x110000; ++cp) out[cp] = s5_class(g_cls[cp]);
}

// suffix letters (in characters) of a contraction that begins at bytes[0]
extern "C" int split5_clen(const uint8_t *bytes, uint32_t len) {
    std::vector<uint8_t> meta(len, 0);
    const PtView v{bytes, meta.data(), len, 0};
    return len ? s5_clen(v, 0) : 0;
}

extern "C" int split5_specials_check(const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t *a, uint32_t *b) {
    return s5_specials_check(bytes, off, n, a, b);
}

// The piece reductions against the per-byte definitions: every meta / aux value a byte can have at every place of a piece,
// among bytes that keep (continuation bytes), for every state in front / value behind.  0 when they agree.
extern "C" int split5_piece_selfcheck() {
    for (uint32_t meta = 0; meta < 256; ++meta)
        for (int k = 0; k < GRP_PIECE; ++k) {
            uint32_t m[4] = {0, 0, 0, 0};
            for (int j = 0; j < GRP_PIECE; ++j) m[j >> 2] |= (uint32_t)(j == k ? meta & ~(uint32_t)PT5_LA : PT_CONT | PT_O) << ((j & 3) * 8);
            const uint8_t mb = (uint8_t)(meta & ~(uint32_t)PT5_LA);
            if (la_piece_state(m) != la_byte(mb)) return 1;
            for (uint32_t after = 0; after < 16; ++after) {
                if ((after & 3u) == 3u || (after >> 2) == 3u) continue;
                uint32_t w[4] = {m[0], m[1], m[2], m[3]};
                la_piece_bits(after, w);
                for (int j = 0; j < GRP_PIECE; ++j) {
                    const uint8_t got = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
                    const uint8_t exp = j == k ? (uint8_t)(mb | la_bit(mb, after)) : (uint8_t)(PT_CONT | PT_O);
                    if (got != exp) return 2;
                }
            }
            if (k & 3) continue; // (the function part: every fourth place, all 65,536 values)
            for (uint32_t aux = 0; aux < 256; ++aux) {
                uint32_t mm[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0};
                for (int j = 0; j < GRP_PIECE; ++j) mm[j >> 2] |= (uint32_t)(j == k ? meta : PT_CONT | PT_O) << ((j & 3) * 8);
                a[k >> 2] = aux << ((k & 3) * 8);
                const S5Fn f = s5_piece_fn(mm, a);
                if (f != s5_fn((uint8_t)meta, (uint8_t)aux)) return 3;
                for (uint8_t s = 0; s < S5_NSTATES; ++s) {
                    bool start;
                    if (s5_apply(f, s) != s5_step(s, (uint8_t)meta, (uint8_t)aux, &start)) return 4;
                    uint32_t o[4] = {a[0], a[1], a[2], a[3]};
                    s5_piece_flags(s, mm, o);
                    for (int j = 0; j < GRP_PIECE; ++j) {
                        // (a continuation byte in the state INS is a byte of the special; the state in front of the bytes
                        // behind k is the one behind k)
                        const uint8_t sj = j <= k ? s : s5_apply(f, s);
                        const uint8_t exp = j == k ? s5_flag(s, (uint8_t)meta, (uint8_t)aux) : sj == S5_INS ? GRP_INSIDE : 0;
                        if ((uint8_t)(o[j >> 2] >> ((j & 3) * 8)) != exp) return 5;
                    }
                }
            }
        }
    // composition: (f g) h == f (g h), and applying a composed function is applying its parts in order
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int it = 0; it < 20000; ++it) {
        const S5Fn f = s5_fn((uint8_t)rnd(), (uint8_t)rnd()), g = s5_fn((uint8_t)rnd(), (uint8_t)rnd()), h = s5_fn((uint8_t)rnd(), (uint8_t)rnd());
        if (s5_then(s5_then(f, g), h) != s5_then(f, s5_then(g, h))) return 6;
        for (uint8_t s = 0; s < S5_NSTATES; ++s)
            if (s5_apply(s5_then(f, g), s) != s5_apply(g, s5_apply(f, s))) return 7;
        if (s5_then(S5_IDENTITY, f) != f || s5_then(f, S5_IDENTITY) != f) return 8;
        const uint32_t a = (uint32_t)rnd() % 3u | ((uint32_t)rnd() % 3u) << 2, b = (uint32_t)rnd() % 3u | ((uint32_t)rnd() % 3u) << 2,
                       c = (uint32_t)rnd() % 3u | ((uint32_t)rnd() % 3u) << 2;
        if (la_comb(la_comb(a, b), c) != la_comb(a, la_comb(b, c))) return 9;
    }
    return 0;
}

static const uint64_t TILE = 256 * 8; // windows per iteration of the carry kernels

struct Words {
    uint32_t m[4], f[4];
};

static Words words(const uint8_t *meta, const uint8_t *flags, uint64_t g, uint64_t n) { // as grp_load of the kernels
    Words p{};
    for (int k = 0; k < GRP_PIECE; ++k) {
        p.m[k >> 2] |= (uint32_t)(g + k < n ? meta[g + k] : (uint8_t)PT_O) << ((k & 3) * 8);
        p.f[k >> 2] |= (uint32_t)(g + k < n && flags ? flags[g + k] : (uint8_t)0) << ((k & 3) * 8);
    }
    return p;
}

static void lookahead_bits(uint8_t *meta, uint64_t n) {
    const uint64_t n_win = (n + GRP_WIN - 1) / GRP_WIN, per_win = GRP_WIN / GRP_PIECE;
    auto state = [&](uint64_t g) { return la_piece_state(words(meta, nullptr, g, n).m); };
    std::vector<uint32_t> win(n_win, 0);
    for (uint64_t w = 0; w < n_win; ++w) {
        uint32_t s = LA_KEEP;
        for (uint64_t t = per_win; t-- > 0;) s = la_comb(s, state(w * GRP_WIN + t * GRP_PIECE));
        win[w] = s;
    }
    const uint64_t n_tiles = (n_win + TILE - 1) / TILE;
    uint32_t carry = LA_KEEP;
    for (uint64_t t = n_tiles; t-- > 0;) { // right to left, the nearest window last
        uint32_t run = carry;
        for (uint64_t w = std::min(n_win, (t + 1) * TILE); w-- > t * TILE;) {
            const uint32_t mine = win[w];
            win[w] = run;
            run = la_comb(run, mine);
        }
        carry = run;
    }
    for (uint64_t w = 0; w < n_win; ++w) {
        uint32_t after = win[w];
        for (uint64_t t = per_win; t-- > 0;) {
            const uint64_t g = w * GRP_WIN + t * GRP_PIECE;
            Words p = words(meta, nullptr, g, n);
            const uint32_t mine = la_piece_state(p.m);
            la_piece_bits(after, p.m);
            for (int k = 0; k < GRP_PIECE && g + k < n; ++k) meta[g + k] = (uint8_t)(p.m[k >> 2] >> ((k & 3) * 8));
            after = la_comb(after, mine);
        }
    }
}

static void function_flags(const uint8_t *meta, uint8_t *flags, uint64_t n) {
    const uint64_t n_win = (n + GRP_WIN - 1) / GRP_WIN, per_win = GRP_WIN / GRP_PIECE;
    auto fn = [&](uint64_t g) {
        const Words p = words(meta, flags, g, n);
        return s5_piece_fn(p.m, p.f);
    };
    std::vector<S5Fn> win(n_win, S5_IDENTITY);
    for (uint64_t w = 0; w < n_win; ++w) {
        S5Fn f = S5_IDENTITY;
        for (uint64_t t = 0; t < per_win; ++t) f = s5_then(f, fn(w * GRP_WIN + t * GRP_PIECE));
        win[w] = f;
    }
    const uint64_t n_tiles = (n_win + TILE - 1) / TILE;
    S5Fn carry = S5_IDENTITY;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        S5Fn run = carry;
        for (uint64_t w = t * TILE; w < std::min(n_win, (t + 1) * TILE); ++w) {
            const S5Fn mine = win[w];
            win[w] = run;
            run = s5_then(run, mine);
        }
        carry = run;
    }
    for (uint64_t w = 0; w < n_win; ++w) {
        S5Fn before = win[w];
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * GRP_WIN + t * GRP_PIECE;
            Words p = words(meta, flags, g, n);
            const S5Fn mine = s5_piece_fn(p.m, p.f);
            s5_piece_flags(s5_apply(before, S5_S0), p.m, p.f); // (whatever stands in front of the text: its first byte is a constant)
            for (int k = 0; k < GRP_PIECE && g + k < n; ++k) flags[g + k] = (uint8_t)(p.f[k >> 2] >> ((k & 3) * 8));
            before = s5_then(before, mine);
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

// flags_out[i] = 1 iff a pre-token of the o200k_base pattern with \p{N}{1,G} starts at byte i.  *err_pos = first malformed byte
// (UnicodeDecodeError.start) or -1.
extern "C" int split5_model(const uint8_t *text, uint64_t n, const uint64_t *chunk_off, uint32_t n_chunks, const uint8_t *sp_bytes,
                            const uint32_t *sp_off, uint32_t n_sp, uint32_t G, uint8_t *flags_out, int64_t *err_pos) {
    build_table();
    std::vector<uint8_t> marks(n, 0), meta(n, 0);
    for (uint32_t c = 0; c < n_chunks; ++c)
        if (chunk_off[c] < n) marks[chunk_off[c]] = PT_CHUNK0;
    *err_pos = -1;
    const PtView v0{text, marks.data(), n, 0};
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t end = n;
        for (uint64_t k = i + 1; k < i + 4 && k < n; ++k)
            if (marks[k] & PT_CHUNK0) {
                end = k;
                break;
            }
        bool bad = false;
        meta[i] = (uint8_t)((marks[i] & PT_CHUNK0) | pt_classify(v0, i, end, g_cls.data(), &bad));
        if (bad && *err_pos < 0) *err_pos = (int64_t)i;
    }
    if (*err_pos >= 0 || n == 0) return 0;
    lookahead_bits(meta.data(), n);
    const PtView v{text, meta.data(), n, 0};
    for (uint64_t i = 0; i < n; ++i) flags_out[i] = s5_aux(v, i);
    if (n_sp) {
        uint32_t max_len = 0;
        for (uint32_t s = 0; s < n_sp; ++s) max_len = std::max(max_len, sp_off[s + 1] - sp_off[s]);
        const PtSpecials sp{sp_bytes, sp_off, n_sp, max_len};
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t o = pt_special_at(v, sp, i);
            if (!o) continue;
            flags_out[i] |= A5_HEAD;
            flags_out[i + pt_special_len(sp, o) - 1] |= A5_LAST;
        }
    }
    function_flags(meta.data(), flags_out, n);
    group_flags(meta.data(), flags_out, n, G);
    return 0;
}
