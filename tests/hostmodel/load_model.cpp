// CPU model of the tile-centric loader (yet-another-bpe_amd/csrc/load_logic.h, k_load_tiles): the kernel's steps run lane by
// lane with the shared arithmetic -- K-ary search for a run's first word, forward walk, byte window in aligned pieces,
// one lane per word -- next to the straightforward per-word loop that k_load_words is.  tests/test_load_model.py compares
// the two (first word of every tile, every slot of every tile, lengths, word bases, long-word list).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../yet-another-bpe_amd/csrc/load_logic.h"

namespace {
constexpr uint32_t CAP = 1024, LMAX = 64, SPAN = CAP - LMAX + 1, LANES = 64;

uint64_t n_tiles_of(const uint64_t *off, uint64_t n_words) {
    const uint64_t packed = (off[n_words] - off[0]) + n_words;
    return (packed + SPAN - 1) / SPAN;
}
}  // namespace

extern "C" {

uint64_t load_model_n_tiles(const uint64_t *off, uint64_t n_words) { return n_tiles_of(off, n_words); }

// ---- the reference: one word at a time into tiles that were filled with PAD first
void load_model_per_word(const uint8_t *bytes, const uint64_t *off, uint64_t n_words, int weighted, uint16_t *tiles, uint32_t *tile_len,
                         uint32_t *tile_wbase, uint32_t *first, uint32_t *long_word, uint64_t *n_long, uint64_t *long_tokens) {
    const uint64_t n_tiles = n_tiles_of(off, n_words), off_base = off[0];
    for (uint64_t i = 0; i < n_tiles * CAP; ++i) tiles[i] = YB_PAD;
    for (uint64_t t = 0; t < n_tiles; ++t) tile_len[t] = 0, tile_wbase[t] = 0xFFFFFFFFu, first[t] = 0xFFFFFFFFu;
    *n_long = *long_tokens = 0;
    for (uint64_t w = 0; w < n_words; ++w) {
        const uint64_t o0 = off[w], L = off[w + 1] - o0;
        const uint64_t pos = (o0 - off_base) + w, tile = pos / SPAN;
        const uint32_t slot = (uint32_t)(pos - tile * SPAN);
        uint16_t *dst = tiles + tile * CAP + slot;
        first[tile] = std::min(first[tile], (uint32_t)w);
        if (weighted) tile_wbase[tile] = std::min(tile_wbase[tile], (uint32_t)w);
        if (!weighted && L <= 1) continue;
        if (L + 1 > LMAX) {
            long_word[(*n_long)++] = (uint32_t)w;
            *long_tokens += L;
            if (weighted) {
                dst[0] = YB_SEP;
                tile_len[tile] = std::max(tile_len[tile], slot + 1);
            }
            continue;
        }
        for (uint32_t j = 0; j < (uint32_t)L; ++j) dst[j] = bytes[o0 + j];
        dst[L] = YB_SEP;
        tile_len[tile] = std::max(tile_len[tile], slot + (uint32_t)L + 1);
    }
}

// ---- the kernel's steps.  Returns 0, or a code if one of the bounds the kernel relies on did not hold.
int load_model_tiled(const uint8_t *bytes, const uint64_t *off, uint64_t n_words, int weighted, uint16_t *tiles, uint32_t *tile_len,
                     uint32_t *tile_wbase, uint32_t *first, uint32_t *long_word, uint64_t *n_long, uint64_t *long_tokens) {
    const uint64_t n_tiles = n_tiles_of(off, n_words), off_base = off[0], off_end = off[n_words];
    const uint32_t pieces = yb_load_window_pieces(SPAN, LMAX);
    std::vector<uint8_t> sb((size_t)pieces * YB_LOAD_STAGE);
    std::vector<uint16_t> img(CAP);
    *n_long = *long_tokens = 0;
    const uint8_t *c_lo = bytes + off_base, *c_hi = bytes + off_end;
    for (uint64_t run0 = 0; run0 < n_tiles; run0 += YB_LOAD_RUN) {  // one wave
        const uint64_t t1 = std::min<uint64_t>(run0 + YB_LOAD_RUN, n_tiles);
        unsigned long long w0 = 0, hi = n_words;
        const unsigned long long target = run0 * SPAN;
        int steps = 0;
        while (w0 < hi) {
            const unsigned long long stride = yb_kary_stride(w0, hi, LANES);
            uint32_t fst = LANES;
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                const unsigned long long w = w0 + lane * stride;
                if (w < hi && yb_load_pos(off[w], off_base, w) >= target) {
                    fst = lane;
                    break;
                }
            }
            yb_kary_narrow(w0, hi, LANES, fst);
            if (++steps > 12) return 1;  // 64^11 > 2^64: the search must be over
        }
        for (uint64_t t = run0; t < t1; ++t) {
            const unsigned long long p0 = t * SPAN, p1 = p0 + SPAN;
            std::fill(img.begin(), img.end(), (uint16_t)YB_PAD);
            std::fill(sb.begin(), sb.end(), (uint8_t)0xAA);  // (what was not fetched must not be used)
            uint32_t len = 0, wbase = 0xFFFFFFFFu;
            unsigned long long o_first = 0;
            bool any = false;
            if (w0 < n_words) {
                o_first = off[w0];
                const unsigned long long pos = yb_load_pos(o_first, off_base, w0);
                if (pos < p0) return 2;  // the walk fell behind
                any = pos < p1;
            }
            first[t] = any ? (uint32_t)w0 : 0xFFFFFFFFu;
            if (any) {
                wbase = (uint32_t)w0;
                const uint8_t *a0 = bytes + o_first;
                const uint8_t *gbase = (const uint8_t *)(uintptr_t)yb_load_window_base((unsigned long long)(uintptr_t)a0);
                for (uint32_t pc = 0; pc < pieces; ++pc) {
                    const uint8_t *g = gbase + (size_t)pc * YB_LOAD_STAGE;
                    if (g >= c_lo && g + YB_LOAD_STAGE <= c_hi) {
                        memcpy(&sb[(size_t)pc * YB_LOAD_STAGE], g, YB_LOAD_STAGE);
                    } else {
                        for (int j = 0; j < YB_LOAD_STAGE; ++j)
                            if (g + j >= c_lo && g + j < c_hi) sb[(size_t)pc * YB_LOAD_STAGE + j] = g[j];
                    }
                }
                const uint32_t sb0 = (uint32_t)(a0 - gbase);
                uint32_t n_in = LANES;
                while (n_in == LANES) {
                    n_in = 0;
                    for (uint32_t lane = 0; lane < LANES; ++lane) {
                        const unsigned long long w = w0 + lane;
                        if (w >= n_words) break;
                        const unsigned long long o0 = off[w], pos = yb_load_pos(o0, off_base, w);
                        if (!(pos >= p0 && pos < p1)) break;
                        ++n_in;
                        const unsigned long long L = off[w + 1] - o0;
                        const YbLoadWord r = yb_load_word(pos, p0, L, weighted != 0, LMAX);
                        if (r.len_end) {
                            if (r.len_end < len) return 3;  // the last word that stores anything ends the tile
                            len = r.len_end;
                        }
                        if (r.kind == YB_LOAD_COPY) {
                            const size_t s = (size_t)sb0 + (size_t)(o0 - o_first);
                            if (s + L > sb.size() || r.slot + L >= CAP) return 4;
                            for (uint32_t j = 0; j < (uint32_t)L; ++j) img[r.slot + j] = sb[s + j];
                            img[r.slot + L] = YB_SEP;
                        } else if (r.kind == YB_LOAD_LONG) {
                            long_word[(*n_long)++] = (uint32_t)w;
                            *long_tokens += L;
                            if (r.sep_only) img[r.slot] = YB_SEP;
                        }
                    }
                    w0 += n_in;
                }
            }
            memcpy(tiles + t * CAP, img.data(), CAP * sizeof(uint16_t));
            tile_len[t] = len;
            tile_wbase[t] = weighted ? wbase : 0xFFFFFFFFu;
        }
    }
    std::sort(long_word, long_word + *n_long);
    return 0;
}

// both forms on one corpus: 0 if everything is equal
int load_model_check(const uint8_t *bytes, const uint64_t *off, uint64_t n_words, int weighted) {
    const uint64_t nt = n_tiles_of(off, n_words);
    std::vector<uint16_t> ta(nt * CAP + 1), tb(nt * CAP + 1);
    std::vector<uint32_t> la(nt + 1), lb(nt + 1), wa(nt + 1), wb(nt + 1), fa(nt + 1), fb(nt + 1), ga(n_words + 1), gb(n_words + 1);
    uint64_t na = 0, nb = 0, ka = 0, kb = 0;
    load_model_per_word(bytes, off, n_words, weighted, ta.data(), la.data(), wa.data(), fa.data(), ga.data(), &na, &ka);
    const int rc = load_model_tiled(bytes, off, n_words, weighted, tb.data(), lb.data(), wb.data(), fb.data(), gb.data(), &nb, &kb);
    if (rc) return rc;
    if (!weighted) std::fill(wa.begin(), wa.end(), 0xFFFFFFFFu);
    if (na != nb || ka != kb) return 10;
    if (!std::equal(ga.begin(), ga.begin() + na, gb.begin())) return 11;
    if (!std::equal(fa.begin(), fa.begin() + nt, fb.begin())) return 12;
    if (!std::equal(la.begin(), la.begin() + nt, lb.begin())) return 13;
    if (!std::equal(wa.begin(), wa.begin() + nt, wb.begin())) return 14;
    if (!std::equal(ta.begin(), ta.begin() + nt * CAP, tb.begin())) return 15;
    return 0;
}

// ---- gathering retile.  kept[t]: the kept elements of old tile t as word lengths with their SEP (words never straddle
// tiles), flattened: tile t has n_words_of[t] words, wlen lists them in stream order.  Both functions fill new_tiles
// (new_n * CAP, PAD elsewhere) and new_len; the element values are their stream numbers mod 65,000, SEP at a word's end.
static uint16_t elem_value(uint64_t g, bool sep) { return sep ? (uint16_t)YB_SEP : (uint16_t)(g % 65000u); }

uint64_t retile_model_new_n(const uint32_t *wlen, uint64_t n_words_total) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_words_total; ++i) total += wlen[i];
    return std::max<uint64_t>(1, (total + SPAN - 1) / SPAN);
}

void retile_model_scatter(const uint32_t *n_words_of, uint64_t n_tiles, const uint32_t *wlen, uint16_t *new_tiles, uint32_t *new_len, uint64_t new_n) {
    for (uint64_t i = 0; i < new_n * CAP; ++i) new_tiles[i] = YB_PAD;
    for (uint64_t i = 0; i < new_n; ++i) new_len[i] = 0;
    uint64_t g = 0, wi = 0;
    for (uint64_t t = 0; t < n_tiles; ++t)
        for (uint32_t k = 0; k < n_words_of[t]; ++k, ++wi) {
            const uint64_t gws = g, nt = gws / SPAN;
            for (uint32_t j = 0; j < wlen[wi]; ++j, ++g) {
                const uint32_t slot = (uint32_t)(g - nt * SPAN);
                new_tiles[nt * CAP + slot] = elem_value(g, j + 1 == wlen[wi]);
                if (j + 1 == wlen[wi]) new_len[nt] = std::max(new_len[nt], slot + 1);
            }
        }
}

int retile_model_gather(const uint32_t *n_words_of, uint64_t n_tiles, const uint32_t *wlen, uint16_t *new_tiles, uint32_t *new_len, uint64_t new_n,
                        uint32_t group) {
    std::vector<unsigned long long> base(n_tiles + 1, 0), wfirst(n_tiles + 1, 0);
    for (uint64_t t = 0, wi = 0; t < n_tiles; ++t) {
        unsigned long long kept = 0;
        for (uint32_t k = 0; k < n_words_of[t]; ++k) kept += wlen[wi++];
        base[t + 1] = base[t] + kept;
        wfirst[t + 1] = wi;
    }
    std::vector<uint8_t> written(new_n, 0);
    for (uint64_t g0 = 0; g0 < new_n; g0 += group) {  // one workgroup
        const unsigned long long k_lo = g0 * SPAN, k_hi = k_lo + (unsigned long long)group * SPAN;
        std::vector<uint16_t> img((size_t)group * CAP, (uint16_t)YB_PAD);
        std::vector<uint32_t> len(group, 0);
        unsigned long long lo = 0, hi = n_tiles;
        int steps = 0;
        while (lo < hi) {
            const unsigned long long stride = yb_kary_stride(lo, hi, LANES);
            uint32_t fst = LANES;
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                const unsigned long long t = lo + lane * stride;
                if (t < hi && base[t + 1] > k_lo) {
                    fst = lane;
                    break;
                }
            }
            yb_kary_narrow(lo, hi, LANES, fst);
            if (++steps > 12) return 1;
        }
        for (uint64_t t = lo; t < n_tiles; ++t) {
            if (base[t] >= k_hi) break;
            unsigned long long g = base[t];
            for (uint64_t wi = wfirst[t]; wi < wfirst[t + 1]; ++wi) {
                const unsigned long long gws = g;
                for (uint32_t j = 0; j < wlen[wi]; ++j, ++g) {
                    const YbGatherDest d = yb_gather_dest(g, gws, k_lo, group, SPAN);
                    if (!d.mine) continue;
                    if (d.tile >= group || d.slot >= CAP || g0 + d.tile >= new_n) return 2;
                    img[(size_t)d.tile * CAP + d.slot] = elem_value(g, j + 1 == wlen[wi]);
                    if (j + 1 == wlen[wi]) len[d.tile] = std::max(len[d.tile], d.slot + 1);
                }
            }
        }
        for (uint32_t k = 0; k < group && g0 + k < new_n; ++k) {
            if (written[g0 + k]++) return 3;
            memcpy(new_tiles + (g0 + k) * CAP, &img[(size_t)k * CAP], CAP * sizeof(uint16_t));
            new_len[g0 + k] = len[k];
        }
    }
    return 0;
}

}  // extern "C"

#ifdef LOAD_MODEL_MAIN
// stand-alone run (for a sanitizer build of the model: g++ -DLOAD_MODEL_MAIN -fsanitize=address,undefined)
#include <stdio.h>
static int run_case(const char *name, const std::vector<uint32_t> &lens, uint64_t off_base) {
    std::vector<uint64_t> off{off_base};
    for (uint32_t L : lens) off.push_back(off.back() + L);
    std::vector<uint8_t> bytes(off.back());  // (exactly the corpus: a read behind it is a heap overflow)
    for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)(i * 131u + 7u);
    for (int weighted = 0; weighted < 2; ++weighted) {
        const int rc = load_model_check(bytes.data(), off.data(), lens.size(), weighted);
        if (rc) {
            printf("%s weighted=%d: code %d\n", name, weighted, rc);
            return 1;
        }
    }
    printf("%s: ok\n", name);
    return 0;
}
int main() {
    int bad = 0;
    bad |= run_case("0 words", {}, 0);
    bad |= run_case("1 word", {5}, 0);
    bad |= run_case("lengths 0 1 2 63 64", {0, 1, 2, 63, 64, 2, 0}, 3);
    bad |= run_case("ends on the last slot of the span", {SPAN - 6, 4, 3}, 0);  // 956 slots, then the 4-byte word: its SEP lies on slot SPAN-1
    bad |= run_case("starts on slot SPAN-1", {62, SPAN - 65, 63, 2}, 17);  // 63 + 897 slots put the third word on slot 960
    bad |= run_case("longer than a span", {3, 2 * SPAN + 100, 4, 5}, 5);
    std::vector<uint32_t> many;
    unsigned long long x = 99;
    for (int i = 0; i < 40000; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        many.push_back((uint32_t)((x >> 33) % 12) + ((x >> 50) % 400 == 0 ? 70 : 0));
    }
    bad |= run_case("about 300 tiles of random words", many, 1001);
    bad |= run_case("single bytes", std::vector<uint32_t>(3000, 0), 0);
    {
        std::vector<uint32_t> nw, wl;
        unsigned long long y = 5;
        for (int t = 0; t < 300; ++t) {
            y = y * 6364136223846793005ull + 1442695040888963407ull;
            uint32_t room = (y >> 40) % 5 == 0 ? 0 : (uint32_t)((y >> 20) % CAP), n = 0;
            while (room >= 2) {
                y = y * 6364136223846793005ull + 1442695040888963407ull;
                const uint32_t L = std::min<uint32_t>(room, 2 + (uint32_t)((y >> 33) % 62));
                wl.push_back(L);
                room -= L;
                ++n;
            }
            nw.push_back(n);
        }
        const uint64_t nn = retile_model_new_n(wl.data(), wl.size());
        std::vector<uint16_t> a(nn * CAP), b(nn * CAP);
        std::vector<uint32_t> la(nn), lb(nn);
        retile_model_scatter(nw.data(), nw.size(), wl.data(), a.data(), la.data(), nn);
        const int rc = retile_model_gather(nw.data(), nw.size(), wl.data(), b.data(), lb.data(), nn, 8);
        const bool ok = rc == 0 && a == b && la == lb;
        printf("gathering retile, %llu new tiles: %s\n", (unsigned long long)nn, ok ? "ok" : "DIFFERENT");
        bad |= !ok;
    }
    return bad;
}
#endif
