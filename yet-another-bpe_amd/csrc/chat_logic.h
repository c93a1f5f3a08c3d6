// chat_logic.h -- the conversation rule (BBPETokenizer.chat_tokens, yet_another_bpe/tokenizer.py), host- and device-callable:
// yabpe_chat_kernels.h and the driver's argument checks call the same functions.
//
// A template gives every role r a header H_r and a footer F_r, a conversation prefix X and, for inference batches, a
// generation prompt G = the header of one named role.  All are id sequences; the content c_t of every turn is encoded as a
// document of its own, so no merge crosses a piece boundary (this is not "render the string, then tokenise it").
//   body_t = H_{r_t} + c_t + F_{r_t}          seq = X + body_0 + ... + body_{T-1} + [G]
// Labels: `ignore` everywhere, but the content and footer ids of a turn whose role is in train_mask carry their own id
// (CHAT_LOSS_ALL: every id of every body; CHAT_LOSS_LAST: only turn T - 1, if its role trains).  X and G never do.
// The cut to max_len (0: none): B = max_len - |X| - |G| > 0 ids are left for the bodies.  Without CHAT_DROP_OLDEST the
// first B ids of the concatenated bodies stay.  With it, q = 1 iff CHAT_PIN_FIRST and T > 0 and r_0 is in pin_mask, else 0;
// L(k) = |body_0 .. body_{q-1}| + |body_k .. body_{T-1}| does not grow with k; k = the smallest value of [q, max(q, T - 1)]
// with L(k) <= B, or max(q, T - 1) if there is none; turns [0, q) and [k, T) stay and are then cut on the right to B.
// No rule reads the batch or another conversation.
#pragma once
#include <stdint.h>

#include "encode_logic.h"  // YB_HD

constexpr uint32_t CHAT_LOSS_ALL = 0x01, CHAT_LOSS_LAST = 0x02, CHAT_DROP_OLDEST = 0x04, CHAT_PIN_FIRST = 0x08, CHAT_GEN_PROMPT = 0x10;  // YABPE_CHAT_*
constexpr uint32_t CHAT_FLAGS = CHAT_LOSS_ALL | CHAT_LOSS_LAST | CHAT_DROP_OLDEST | CHAT_PIN_FIRST | CHAT_GEN_PROMPT;
constexpr uint32_t CHAT_MAX_ROLES = 16;       // YABPE_CHAT_MAX_ROLES
constexpr uint32_t CHAT_MAX_TPL = 2048;       // ids of X, every header and every footer together: what the write pass holds in LDS
constexpr uint32_t CHAT_BLOCK = 256;          // threads of every chat kernel
constexpr uint32_t CHAT_SLOTS = 4;            // consecutive output slots a lane of the write pass owns (one 16-byte store each way)
constexpr uint32_t CHAT_TILE = CHAT_BLOCK * CHAT_SLOTS;  // output slots a workgroup of the write pass owns
constexpr uint32_t CHAT_STAGE = CHAT_BLOCK;   // turn records the write pass holds in LDS at a time
constexpr unsigned long long CHAT_MAX_CONV = 0xFFFFFFFFull;  // ids of one conversation at most
constexpr uint32_t CHAT_BAD_ROLE = 0x1, CHAT_TOO_LONG = 0x2;  // what the plan passes raise

// the rule's argument checks; n_gen: the length of G (0 without CHAT_GEN_PROMPT)
YB_HD bool chat_rule_valid(uint32_t n_roles, uint32_t flags, uint32_t gen_role, unsigned long long max_len, unsigned long long n_prefix,
                           unsigned long long n_gen) {
    if (n_roles < 1 || n_roles > CHAT_MAX_ROLES) return false;
    if (flags & ~CHAT_FLAGS) return false;
    if ((flags & CHAT_LOSS_ALL) && (flags & CHAT_LOSS_LAST)) return false;
    if ((flags & CHAT_GEN_PROMPT) && gen_role >= n_roles) return false;
    if (max_len != 0 && max_len <= n_prefix + n_gen) return false;
    return true;
}

YB_HD unsigned long long chat_turn_len(uint32_t head, unsigned long long content, uint32_t foot) { return (unsigned long long)head + content + foot; }

// q of a conversation of T turns whose first role is r0
YB_HD uint32_t chat_pinned(uint32_t flags, unsigned long long T, uint32_t r0, uint32_t pin_mask) {
    return (flags & CHAT_DROP_OLDEST) && (flags & CHAT_PIN_FIRST) && T > 0 && ((pin_mask >> r0) & 1u) ? 1u : 0u;
}

// L(k) of the conversation with turns [t0, t1), from Gs = the exclusive prefix sums of the turn lengths
YB_HD unsigned long long chat_kept_len(const unsigned long long *Gs, unsigned long long t0, unsigned long long t1, uint32_t q, unsigned long long k) {
    return (Gs[t0 + q] - Gs[t0]) + (Gs[t1] - Gs[t0 + k]);
}

// k: the smallest value of [q, max(q, T - 1)] with L(k) <= B, else max(q, T - 1) -- a binary search, L does not grow with k
YB_HD unsigned long long chat_pick_k(const unsigned long long *Gs, unsigned long long t0, unsigned long long t1, uint32_t q, unsigned long long B) {
    const unsigned long long T = t1 - t0;
    unsigned long long lo = q, hi = T > (unsigned long long)q + 1 ? T - 1 : q;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (chat_kept_len(Gs, t0, t1, q, mid) <= B) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The ids turn t0 + j keeps: it stays whole, is dropped (q <= j < k) or is shortened by the right cut to B (B = ~0: no cut).
YB_HD unsigned long long chat_turn_kept(const unsigned long long *Gs, unsigned long long t0, unsigned long long j, uint32_t q, unsigned long long k,
                                        unsigned long long B) {
    if (j >= q && j < k) return 0;
    const unsigned long long at = j < q ? Gs[t0 + j] - Gs[t0] : (Gs[t0 + q] - Gs[t0]) + (Gs[t0 + j] - Gs[t0 + k]);  // ids kept before it
    const unsigned long long len = Gs[t0 + j + 1] - Gs[t0 + j];
    return at >= B ? 0 : (B - at < len ? B - at : len);
}

// does turn j of T (role r) carry labels at all?
YB_HD bool chat_turn_trains(uint32_t flags, uint32_t train_mask, uint32_t r, unsigned long long j, unsigned long long T) {
    if (flags & CHAT_LOSS_ALL) return true;
    if ((flags & CHAT_LOSS_LAST) && j + 1 != T) return false;
    return ((train_mask >> r) & 1u) != 0;
}

enum ChatPart : uint32_t { CHAT_HEADER = 0, CHAT_CONTENT = 1, CHAT_FOOTER = 2 };

// position p inside a body with a header of `head` and a content of `content` ids -> the part, *idx = the index inside it
YB_HD uint32_t chat_part(unsigned long long p, uint32_t head, unsigned long long content, unsigned long long *idx) {
    if (p < head) {
        *idx = p;
        return CHAT_HEADER;
    }
    if (p - head < content) {
        *idx = p - head;
        return CHAT_CONTENT;
    }
    *idx = p - head - content;
    return CHAT_FOOTER;
}

// does an id of this part carry a label, in a turn that trains?
YB_HD bool chat_labelled(bool trains, uint32_t part, uint32_t flags) { return trains && ((flags & CHAT_LOSS_ALL) || part != CHAT_HEADER); }
