// fim_logic.h -- the fill-in-the-middle rule (BBPETokenizer.fim_tokens / fim_cuts, yet_another_bpe/tokenizer.py), host- and
// device-callable: yabpe_fim_kernels.h and the CPU model of tests/hostmodel/fim_model.cpp call the same functions.
//
// With rnd(seed, stream, i) of yet_another_bpe/synth.py (enc_rnd of encode_logic.h) and T(x) = min(2^32, int(x * 2^32)):
// document d of the batch has the key Kd = rnd(seed, 0x66, first_doc + d) -- a stream of its own, so one seed gives draws
// unrelated to the mask's and the span pass's.  r = rnd(Kd, 0x61, 0): the document is transformed iff (r >> 32) < Tf, and a
// transformed one is SPM iff (r & 0xFFFFFFFF) < Ts, else PSM.  With n units in the document (ids at token level, code points
// of the normalised text at character level) x = rnd(Kd, 0x62, 0) % (n + 1), y = rnd(Kd, 0x62, 1) % (n + 1), a = min(x, y),
// b = max(x, y): prefix = units [0, a), middle = [a, b), suffix = [b, n).  A document left alone has a = b = n.  No draw reads
// the batch, the row length or another document.
//
// A document is a contiguous run of ids with the two cut points (a, b) in it -- drawn here at token level, or the lengths of
// its three separately encoded pieces at character level -- so both levels share the plan and the write:
//   PSM  pre P suf S mid M [eot]        SPM  pre suf S mid P M [eot]        left alone: its ids
// The cut to max_len (0: none) takes the excess over max_len - (3 + eot) from the end of the suffix, then from the start of
// the prefix, then from the end of the middle; the sentinels always survive.  A document left alone keeps its first max_len ids.
#pragma once
#include <stdint.h>

#include "encode_logic.h"
#include "mask_logic.h"  // mask_doc_of

constexpr unsigned long long FIM_STREAM_DOC = 0x66, FIM_STREAM_MODE = 0x61, FIM_STREAM_CUT = 0x62;
constexpr unsigned long long FIM_T_ONE = 1ull << 32;  // T of 1.0
constexpr uint32_t FIM_BLOCK = 256;                   // output slots a workgroup of the write pass takes
constexpr uint32_t FIM_EOT = 0x1, FIM_LOSS_MIDDLE = 0x2, FIM_PIECES = 0x4;  // YABPE_FIM_*
constexpr uint32_t FIM_FLAGS = FIM_EOT | FIM_LOSS_MIDDLE | FIM_PIECES;
constexpr unsigned long long FIM_MAX_DOC = 0xFFFFFFFFull;  // ids of one document at most

enum FimMode : uint32_t { FIM_NONE = 0, FIM_PSM = 1, FIM_SPM = 2 };

struct FimRule {
    unsigned long long fim, spm;  // Tf, Ts <= 2^32
    uint32_t pre_id, suf_id, mid_id, eot_id, ignore;
    unsigned long long max_len;   // 0: no cut
    uint32_t flags;               // FIM_*
};

// a document after the cut: the kept lengths, and where the kept prefix and the suffix start among the document's ids
struct FimDoc {
    uint32_t mode, p, m, s;
    uint32_t dp, b;  // the kept prefix is ids [dp, dp + p), the kept middle [dp + p, dp + p + m), the kept suffix [b, b + s)
};

YB_HD unsigned long long fim_extra(uint32_t flags) { return 3ull + ((flags & FIM_EOT) ? 1ull : 0ull); }  // X

// the rule's argument checks (yabpe_fim, yabpe_fim_cuts and the model refuse the same things)
YB_HD bool fim_rule_valid(unsigned long long fim, unsigned long long spm, unsigned long long max_len, uint32_t flags) {
    if (fim > FIM_T_ONE || spm > FIM_T_ONE) return false;
    if (flags & ~FIM_FLAGS) return false;
    if (max_len != 0 && max_len <= fim_extra(flags)) return false;
    return true;
}

YB_HD unsigned long long fim_doc_key(unsigned long long seed, unsigned long long first_doc, unsigned long long d) {
    return enc_rnd(seed, FIM_STREAM_DOC, first_doc + d);
}

YB_HD uint32_t fim_mode(unsigned long long kd, unsigned long long Tf, unsigned long long Ts) {
    const unsigned long long r = enc_rnd(kd, FIM_STREAM_MODE, 0);
    if ((r >> 32) >= Tf) return FIM_NONE;
    return (r & 0xFFFFFFFFull) < Ts ? FIM_SPM : FIM_PSM;
}

// the cut points of a document of n units (n <= 2^32 - 1 at token level; any n at character level)
YB_HD void fim_draw_cuts(unsigned long long kd, uint32_t mode, unsigned long long n, unsigned long long *a, unsigned long long *b) {
    if (mode == FIM_NONE) {
        *a = *b = n;
        return;
    }
    const unsigned long long x = enc_rnd(kd, FIM_STREAM_CUT, 0) % (n + 1), y = enc_rnd(kd, FIM_STREAM_CUT, 1) % (n + 1);
    *a = x < y ? x : y;
    *b = x < y ? y : x;
}

// The plan of one document: its n ids with the cut points a <= b <= n and its mode -> what is kept; *out_len = the slots of
// its sequence, *dropped = the ids the cut removes.
YB_HD FimDoc fim_plan(uint32_t mode, unsigned long long n, unsigned long long a, unsigned long long b, const FimRule &R, unsigned long long *out_len,
                      unsigned long long *dropped) {
    unsigned long long p = a, m = b - a, s = n - b, dp = 0;
    if (mode == FIM_NONE) {  // the first max_len ids of the whole run
        unsigned long long e = (R.max_len && n > R.max_len) ? n - R.max_len : 0;
        *dropped = e;
        unsigned long long t = e < s ? e : s;
        s -= t, e -= t;
        t = e < m ? e : m;
        m -= t, e -= t;
        p -= e;
        *out_len = p + m + s;
    } else {
        const unsigned long long X = fim_extra(R.flags);
        unsigned long long e = 0;
        if (R.max_len) {
            const unsigned long long C = R.max_len - X;  // >= 1: fim_rule_valid
            if (n > C) e = n - C;
        }
        *dropped = e;
        unsigned long long t = e < s ? e : s;  // the end of the suffix
        s -= t, e -= t;
        t = e < p ? e : p;                     // the start of the prefix
        p -= t, dp = t, e -= t;
        m -= e;                                // the end of the middle (e < m: C >= 1)
        *out_len = X + p + m + s;
    }
    return FimDoc{mode, (uint32_t)p, (uint32_t)m, (uint32_t)s, (uint32_t)dp, (uint32_t)b};
}

// what stands in slot k of a document's sequence
enum FimSlot : uint32_t { FIM_SLOT_PREFIX = 0, FIM_SLOT_MIDDLE = 1, FIM_SLOT_SUFFIX = 2, FIM_SLOT_SENTINEL = 3, FIM_SLOT_EOT = 4 };

// Slot k (below the document's out_len) -> its kind; *src = for the three content kinds the index of the id among the
// document's ids, for the other two the id itself.  At most seven comparisons: no loop.
YB_HD uint32_t fim_slot(const FimDoc &D, unsigned long long k, const FimRule &R, unsigned long long *src) {
    const unsigned long long p = D.p, m = D.m, s = D.s, a = (unsigned long long)D.dp + p;
    if (D.mode == FIM_NONE) {  // (the kept ids are the first p + m + s of the run)
        *src = k;
        return k < p ? FIM_SLOT_PREFIX : k < p + m ? FIM_SLOT_MIDDLE : FIM_SLOT_SUFFIX;
    }
    if (k == 0) {
        *src = R.pre_id;
        return FIM_SLOT_SENTINEL;
    }
    if (k == 3 + p + m + s) {
        *src = R.eot_id;
        return FIM_SLOT_EOT;
    }
    if (k >= 3 + p + s) {  // both orders end with the middle
        *src = a + (k - 3 - p - s);
        return FIM_SLOT_MIDDLE;
    }
    if (D.mode == FIM_PSM) {  // pre P suf S mid
        if (k < 1 + p) {
            *src = D.dp + (k - 1);
            return FIM_SLOT_PREFIX;
        }
        if (k == 1 + p) {
            *src = R.suf_id;
            return FIM_SLOT_SENTINEL;
        }
        if (k < 2 + p + s) {
            *src = D.b + (k - 2 - p);
            return FIM_SLOT_SUFFIX;
        }
        *src = R.mid_id;
        return FIM_SLOT_SENTINEL;
    }
    // pre suf S mid P
    if (k == 1) {
        *src = R.suf_id;
        return FIM_SLOT_SENTINEL;
    }
    if (k < 2 + s) {
        *src = D.b + (k - 2);
        return FIM_SLOT_SUFFIX;
    }
    if (k == 2 + s) {
        *src = R.mid_id;
        return FIM_SLOT_SENTINEL;
    }
    *src = D.dp + (k - 3 - s);
    return FIM_SLOT_PREFIX;
}

// does a slot of this kind in a document of this mode carry a label?
YB_HD bool fim_labelled(uint32_t mode, uint32_t kind, uint32_t flags) {
    return !(flags & FIM_LOSS_MIDDLE) || mode == FIM_NONE || kind == FIM_SLOT_MIDDLE || kind == FIM_SLOT_EOT;
}

// One output slot in full: document d's plan, its first id at ids[first] -> *id, *label
YB_HD void fim_write_slot(const FimDoc &D, unsigned long long k, const uint32_t *ids, unsigned long long first, const FimRule &R, uint32_t *id,
                          uint32_t *label) {
    unsigned long long src;
    const uint32_t kind = fim_slot(D, k, R, &src);
    const uint32_t v = kind <= FIM_SLOT_SUFFIX ? ids[first + src] : (uint32_t)src;
    *id = v;
    *label = fim_labelled(D.mode, kind, R.flags) ? v : R.ignore;
}

// ---------------------------------------------------------------- character-level cuts on UTF-8 text
// table[g] = the non-continuation bytes below g * granule (n_gran + 1 entries).  lead(p) for any granule (the model runs small
// ones; the kernels run ENC_GRANULE through enc_lead's 16-byte chunks).
YB_HD unsigned long long fim_lead(const uint8_t *text, const unsigned long long *table, uint32_t granule, unsigned long long p) {
    const unsigned long long g = p / granule;
    unsigned long long r = table[g];
    for (unsigned long long c = g * granule; c < p; ++c) r += enc_is_lead(text[c]) ? 1u : 0u;
    return r;
}

// The byte position of the lead byte with global index t (t below table[g_hi + 1]; the answer lies in a granule of [g_lo,
// g_hi]): a search of the table, then at most one granule of bytes.  end: no byte at or past it is read.
YB_HD unsigned long long fim_select(const uint8_t *text, unsigned long long end, const unsigned long long *table, uint32_t granule,
                                    unsigned long long g_lo, unsigned long long g_hi, unsigned long long t) {
    while (g_lo < g_hi) {  // the last g with table[g] <= t
        const unsigned long long mid = g_lo + (g_hi - g_lo + 1) / 2;
        if (table[mid] <= t) g_lo = mid; else g_hi = mid - 1;
    }
    unsigned long long left = t - table[g_lo], c = g_lo * granule;
    const unsigned long long stop = c + granule < end ? c + granule : end;
    for (; c < stop; ++c)
        if (enc_is_lead(text[c])) {
            if (left == 0) return c;
            --left;
        }
    return end;  // (not reached with t below the leads of [g_lo, g_hi])
}

// One document's cuts: its bytes [start, end), lead_start / lead_end = lead(start) / lead(end) -> mode, (a, b) in characters,
// and the byte starts of the middle and the suffix.
YB_HD void fim_doc_cuts(const uint8_t *text, const unsigned long long *table, uint32_t granule, unsigned long long start, unsigned long long end,
                        unsigned long long lead_start, unsigned long long lead_end, unsigned long long kd, unsigned long long Tf,
                        unsigned long long Ts, unsigned long long *cuts3, unsigned long long *piece3) {
    const unsigned long long n = lead_end - lead_start;
    const uint32_t mode = fim_mode(kd, Tf, Ts);
    unsigned long long a, b;
    fim_draw_cuts(kd, mode, n, &a, &b);
    cuts3[0] = mode, cuts3[1] = a, cuts3[2] = b;
    const unsigned long long g_lo = start / granule, g_hi = end > start ? (end - 1) / granule : g_lo;
    piece3[0] = start;
    piece3[1] = a < n ? fim_select(text, end, table, granule, g_lo, g_hi, lead_start + a) : end;
    piece3[2] = b < n ? fim_select(text, end, table, granule, g_lo, g_hi, lead_start + b) : end;
}
