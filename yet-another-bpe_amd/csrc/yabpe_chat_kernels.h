// yabpe_chat_kernels.h -- conversation batches for supervised fine-tuning: every conversation written through a chat template
// as X + (H_r + content + F_r per kept turn) + [G], with labels on the assistant's turns only and the cut to max_len by whole
// turns (rule in chat_logic.h; contract: BBPETokenizer.chat_tokens, yet_another_bpe/tokenizer.py).
//
// Records.  The output stream is a sequence of RECORDS: one per turn, plus one pseudo-turn at the end of every conversation.
// Conversation c with turns [t0, t1) owns records [t0 + c, t1 + c]; record t + c is turn t, record t1 + c the pseudo-turn.
// The pseudo-turn is a turn of role gen_role with an empty content and no footer whose header is G (nothing without
// CHAT_GEN_PROMPT) and that never trains.  X is charged to the conversation's first record -- its first turn, kept or
// dropped, or with T = 0 the pseudo-turn -- so a conversation without turns needs no case of its own anywhere.
//
// Passes (host orchestration: yabpe_chat in yabpe.hip):
//   len    k_chat_turn_len: one thread per TURN.  |H_r| + content + |F_r|, the content from the encoder's doc_off; a role past
//          n_roles raises CHAT_BAD_ROLE.  One exclusive_scan over the n_turns lengths gives Gs, and every L(k) is then two
//          subtractions (chat_kept_len): no backward or segmented scan.
//   plan   k_chat_plan: one thread per CONVERSATION.  q, and k by a binary search over Gs inside the conversation's turns
//          (chat_pick_k); a conversation past 2^32 - 1 ids raises CHAT_TOO_LONG.
//   kept   k_chat_kept: one thread per RECORD.  Its conversation by a search of conv_off, the kept length (0 for a dropped
//          turn, the last kept turn shortened by the right cut, X and G charged as above) and the record the write pass reads:
//          content start, the three lengths, role, the label bit, the conversation.  A second exclusive_scan gives O, the
//          start of every record in the output; O is monotone and a dropped turn is an empty interval.
//   write  k_chat_write: a workgroup owns CHAT_TILE consecutive output slots, a lane CHAT_SLOTS consecutive ones.  One
//          search in O finds the first record that reaches into the tile; the records that cover the tile are staged into LDS
//          CHAT_STAGE at a time (a tile of one-id turns holds more records than one stage: rounds), starts relative to the
//          tile; the template is staged once.  A lane finds the record of its first slot by a search in LDS and walks on from
//          there, takes template ids from LDS and content ids from global memory -- one 16-byte load when its four slots lie
//          in one aligned content run, else four 4-byte loads that the wave's neighbours share lines with -- and stores ids
//          and labels with one 16-byte store each.  The labels of a conversation are counted per wave by ballots and added
//          with one atomic per wave and conversation present in it.
//   finish k_chat_finish: one thread per CONVERSATION.  The conversation offsets (O at its first record), the kept ids into
//          info, and the call's counters, summed per wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chat_logic.h"

namespace yb {

constexpr uint32_t CHAT_TPL_HDR = 2 * (CHAT_MAX_ROLES + 1);  // the template table: 17 header starts, 17 footer starts, then the ids (X first)
constexpr uint32_t CHAT_REC_ROLE = 0x1F, CHAT_REC_TRAINS = 0x100, CHAT_REC_FIRST = 0x200;  // meta word of a record
enum ChatCounter : uint32_t { CHAT_C_DROPPED = 0, CHAT_C_CUT = 1, CHAT_C_LABELLED = 2, CHAT_C_UNLABELLED = 3, CHAT_COUNTERS = 4 };

struct ChatParams {
    const uint32_t *ids;                 // 16-byte aligned
    unsigned long long n_ids;
    const unsigned long long *doc_off;   // n_turns content starts (ids), ascending, doc_off[0] = 0
    uint32_t n_turns, n_convs;
    const unsigned long long *conv_off;  // n_convs + 1 turn offsets, the last one n_turns
    const uint8_t *roles;                // [n_turns]
    const uint32_t *tpl;                 // [CHAT_TPL_HDR + n_tpl]: where H_r and F_r start in this table, then X, the headers, the footers
    uint32_t n_tpl, n_x, n_g, n_roles, gen_role;
    uint32_t train_mask, pin_mask, ignore, flags;
    unsigned long long B;                // ids left for the bodies; ~0: no cut
    unsigned long long n_rec;            // n_turns + n_convs
    unsigned long long *len;             // [n_turns] then, reused, [n_rec]: turn lengths / kept lengths of the records
    unsigned long long *Gs;              // [n_turns + 1]
    unsigned long long *O;               // [n_rec + 1]
    uint4 *rec4;                         // [n_rec]: content start (lo, hi), content length, |H| | |F| << 16
    uint2 *rec2;                         // [n_rec]: conversation, meta
    uint32_t *status;                    // CHAT_BAD_ROLE | CHAT_TOO_LONG
    uint4 *info;                         // [n_convs]: (q, k, ids kept, ids with a label)
    unsigned long long *out_off;         // [n_convs + 1]
    unsigned long long n_out;
    uint32_t *out_ids, *out_labels;
    unsigned long long *counters;        // [CHAT_COUNTERS]
};

__device__ __forceinline__ uint32_t chat_head_len(const uint32_t *tpl, uint32_t r) { return tpl[r + 1] - tpl[r]; }
__device__ __forceinline__ uint32_t chat_foot_len(const uint32_t *tpl, uint32_t r) { return tpl[CHAT_MAX_ROLES + 2 + r] - tpl[CHAT_MAX_ROLES + 1 + r]; }

__global__ __launch_bounds__(CHAT_BLOCK) void k_chat_turn_len(ChatParams P) {
    const unsigned long long t = (unsigned long long)blockIdx.x * CHAT_BLOCK + threadIdx.x;
    if (t >= P.n_turns) return;
    const uint32_t r = P.roles[t];
    if (r >= P.n_roles) {  // (the call fails; the turn counts nothing, so nothing below reads past the template)
        atomicOr(P.status, CHAT_BAD_ROLE);
        P.len[t] = 0;
        return;
    }
    const unsigned long long content = (t + 1 < P.n_turns ? P.doc_off[t + 1] : P.n_ids) - P.doc_off[t];
    P.len[t] = chat_turn_len(chat_head_len(P.tpl, r), content, chat_foot_len(P.tpl, r));
}

__global__ __launch_bounds__(CHAT_BLOCK) void k_chat_plan(ChatParams P) {
    const unsigned long long c = (unsigned long long)blockIdx.x * CHAT_BLOCK + threadIdx.x;
    if (c >= P.n_convs) return;
    const unsigned long long t0 = P.conv_off[c], t1 = P.conv_off[c + 1], T = t1 - t0;
    if ((unsigned long long)P.n_x + (P.Gs[t1] - P.Gs[t0]) + P.n_g > CHAT_MAX_CONV) atomicOr(P.status, CHAT_TOO_LONG);
    const uint32_t r0 = T ? P.roles[t0] : 0;
    const uint32_t q = chat_pinned(P.flags, T, r0 < 32 ? r0 : 31, P.pin_mask);
    const unsigned long long k = (P.flags & CHAT_DROP_OLDEST) && P.B != ~0ull ? chat_pick_k(P.Gs, t0, t1, q, P.B) : q;
    P.info[c] = make_uint4(q, (uint32_t)k, 0, 0);
}

__global__ __launch_bounds__(CHAT_BLOCK) void k_chat_kept(ChatParams P) {
    const unsigned long long r = (unsigned long long)blockIdx.x * CHAT_BLOCK + threadIdx.x;
    if (r >= P.n_rec) return;
    unsigned long long lo = 0, hi = P.n_convs - 1;  // the last conversation whose first record is at or below r
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo + 1) / 2;
        if (P.conv_off[mid] + mid <= r) lo = mid; else hi = mid - 1;
    }
    const unsigned long long c = lo, t = r - c, t0 = P.conv_off[c], t1 = P.conv_off[c + 1];
    const bool first = t == t0;
    unsigned long long kept = first ? P.n_x : 0, src = 0;
    uint32_t content = 0, lens = 0, meta = first ? CHAT_REC_FIRST : 0;
    if (t == t1) {  // the pseudo-turn: G as the header of a turn that never trains
        kept += P.n_g;
        lens = P.n_g;
        meta |= P.gen_role;
    } else {
        const uint32_t role = P.roles[t];
        const uint4 f = P.info[c];
        kept += chat_turn_kept(P.Gs, t0, t - t0, f.x, f.y, P.B);
        if (role < P.n_roles) {
            src = P.doc_off[t];
            content = (uint32_t)((t + 1 < P.n_turns ? P.doc_off[t + 1] : P.n_ids) - src);
            lens = chat_head_len(P.tpl, role) | chat_foot_len(P.tpl, role) << 16;
            meta |= role | (chat_turn_trains(P.flags, P.train_mask, role, t - t0, t1 - t0) ? CHAT_REC_TRAINS : 0);
        }
    }
    P.len[r] = kept;
    P.rec4[r] = make_uint4((uint32_t)src, (uint32_t)(src >> 32), content, lens);
    P.rec2[r] = make_uint2((uint32_t)c, meta);
}

__device__ __forceinline__ uint32_t chat_rel(unsigned long long o, unsigned long long tile0) {  // where o lies in the tile, clamped
    return o <= tile0 ? 0u : (o - tile0 < CHAT_TILE ? (uint32_t)(o - tile0) : CHAT_TILE);
}

__global__ __launch_bounds__(CHAT_BLOCK) void k_chat_write(ChatParams P) {
    __shared__ uint32_t s_tpl[CHAT_TPL_HDR + CHAT_MAX_TPL];
    __shared__ uint32_t s_start[CHAT_STAGE + 1];  // of each staged record the slot of the tile it starts in; [CHAT_STAGE]: where the next stage starts
    __shared__ uint32_t s_skip[CHAT_STAGE];       // the ids of the record that lie before the tile
    __shared__ uint4 s_rec4[CHAT_STAGE];
    __shared__ uint2 s_rec2[CHAT_STAGE];
    __shared__ unsigned long long s_first;
    const uint32_t tid = threadIdx.x;
    const unsigned long long tile0 = (unsigned long long)blockIdx.x * CHAT_TILE;  // (tile0 < n_out: the grid)
    const uint32_t tile_n = P.n_out - tile0 < CHAT_TILE ? (uint32_t)(P.n_out - tile0) : CHAT_TILE;
    for (uint32_t k = tid; k < CHAT_TPL_HDR + P.n_tpl; k += CHAT_BLOCK) s_tpl[k] = P.tpl[k];
    if (tid == 0) {  // the last record that starts at or before the tile: it is not empty, O[n_rec] = n_out > tile0
        unsigned long long lo = 0, hi = P.n_rec - 1;
        while (lo < hi) {
            const unsigned long long mid = lo + (hi - lo + 1) / 2;
            if (P.O[mid] <= tile0) lo = mid; else hi = mid - 1;
        }
        s_first = lo;
    }
    __syncthreads();
    const unsigned long long r_first = s_first;
    const uint32_t i0 = tid * CHAT_SLOTS;
    uint32_t id[CHAT_SLOTS] = {0, 0, 0, 0}, conv[CHAT_SLOTS] = {0, 0, 0, 0};
    unsigned long long g[CHAT_SLOTS] = {0, 0, 0, 0};  // of a content slot: where its id lies in ids
    uint32_t from_ids = 0, lab = 0;                   // a bit per slot: a content id; carries a label
    for (unsigned long long rb = r_first;; rb += CHAT_STAGE) {
        {   // a stage: records [rb, rb + CHAT_STAGE); past the last record everything starts at n_out
            const unsigned long long r = rb + tid, o = r <= P.n_rec ? P.O[r] : P.n_out;
            s_start[tid] = chat_rel(o, tile0);
            s_skip[tid] = o < tile0 ? (uint32_t)(tile0 - o) : 0u;
            if (r < P.n_rec) {
                s_rec4[tid] = P.rec4[r];
                s_rec2[tid] = P.rec2[r];
            }
            if (tid == 0) s_start[CHAT_STAGE] = chat_rel(rb + CHAT_STAGE <= P.n_rec ? P.O[rb + CHAT_STAGE] : P.n_out, tile0);
        }
        __syncthreads();
        const uint32_t from = s_start[0], to = s_start[CHAT_STAGE];  // the slots this stage covers (to <= tile_n)
        uint32_t j = 0;
        bool have = false;
#pragma unroll
        for (uint32_t s = 0; s < CHAT_SLOTS; ++s) {
            const uint32_t i = i0 + s;
            if (i < from || i >= to) continue;
            if (!have || s_start[j + 1] <= i) {  // the last staged record that starts at or before slot i (empty ones are passed over)
                uint32_t lo = have ? j + 1 : 0, hi = CHAT_STAGE - 1;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo + 1) / 2;
                    if (s_start[mid] <= i) lo = mid; else hi = mid - 1;
                }
                j = lo;
                have = true;
            }
            const uint4 a = s_rec4[j];
            const uint2 b = s_rec2[j];
            unsigned long long p = (unsigned long long)(i - s_start[j]) + s_skip[j];  // the position inside the record
            conv[s] = b.x;
            if ((b.y & CHAT_REC_FIRST) && p < P.n_x) {
                id[s] = s_tpl[CHAT_TPL_HDR + p];
                continue;
            }
            if (b.y & CHAT_REC_FIRST) p -= P.n_x;
            unsigned long long idx;
            const uint32_t part = chat_part(p, a.w & 0xFFFFu, a.z, &idx), role = b.y & CHAT_REC_ROLE;
            if (chat_labelled((b.y & CHAT_REC_TRAINS) != 0, part, P.flags)) lab |= 1u << s;
            if (part == CHAT_CONTENT) {
                g[s] = ((unsigned long long)a.y << 32 | a.x) + idx;
                from_ids |= 1u << s;
            } else {
                id[s] = s_tpl[s_tpl[(part == CHAT_FOOTER ? CHAT_MAX_ROLES + 1 : 0) + role] + (uint32_t)idx];
            }
        }
        if (to >= tile_n) break;  // (the same for every thread)
        __syncthreads();
    }
    if (from_ids == 0xFu && g[3] == g[0] + 3 && (g[0] & 3) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.ids + g[0]);
        id[0] = v.x, id[1] = v.y, id[2] = v.z, id[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t s = 0; s < CHAT_SLOTS; ++s)
            if (from_ids >> s & 1u) id[s] = P.ids[g[s]];
    }
    uint32_t label[CHAT_SLOTS];
#pragma unroll
    for (uint32_t s = 0; s < CHAT_SLOTS; ++s) label[s] = (lab >> s & 1u) ? id[s] : P.ignore;
    if (i0 + CHAT_SLOTS <= tile_n) {
        *reinterpret_cast<uint4 *>(P.out_ids + tile0 + i0) = make_uint4(id[0], id[1], id[2], id[3]);
        *reinterpret_cast<uint4 *>(P.out_labels + tile0 + i0) = make_uint4(label[0], label[1], label[2], label[3]);
    } else {
#pragma unroll
        for (uint32_t s = 0; s < CHAT_SLOTS; ++s)
            if (i0 + s < tile_n) {
                P.out_ids[tile0 + i0 + s] = id[s];
                P.out_labels[tile0 + i0 + s] = label[s];
            }
    }
    // the labels per conversation: the wave takes one conversation with labels left at a time
    const uint32_t lane = tid & 63u;
    for (;;) {
        const unsigned long long open = __ballot(lab != 0);
        if (!open) break;
        const int leader = __ffsll((long long)open) - 1;
        const uint32_t mine = (lab & 1u) ? conv[0] : (lab & 2u) ? conv[1] : (lab & 4u) ? conv[2] : conv[3];
        const uint32_t c = __shfl(mine, leader);
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t s = 0; s < CHAT_SLOTS; ++s)
            if ((lab >> s & 1u) && conv[s] == c) {
                ++cnt;
                lab &= ~(1u << s);
            }
        const uint32_t total = __popcll(__ballot(cnt & 1u)) + 2 * __popcll(__ballot(cnt & 2u)) + 4 * __popcll(__ballot(cnt & 4u));
        if ((int)lane == leader) atomicAdd(&P.info[c].w, total);
    }
}

__global__ __launch_bounds__(CHAT_BLOCK) void k_chat_finish(ChatParams P) {
    const unsigned long long c = (unsigned long long)blockIdx.x * CHAT_BLOCK + threadIdx.x;
    unsigned long long cnt[CHAT_COUNTERS] = {0, 0, 0, 0};
    if (c <= P.n_convs) {
        const unsigned long long at = P.O[P.conv_off[c] + c];  // (conv_off[n_convs] + n_convs = n_rec)
        P.out_off[c] = at;
        if (c < P.n_convs) {
            const unsigned long long t0 = P.conv_off[c], t1 = P.conv_off[c + 1], kept = P.O[t1 + c + 1] - at;
            const uint4 f = P.info[c];
            P.info[c].z = (uint32_t)kept;
            cnt[CHAT_C_DROPPED] = f.y - f.x;
            cnt[CHAT_C_CUT] = P.n_x + (P.Gs[t1] - P.Gs[t0]) + P.n_g - kept;
            cnt[CHAT_C_LABELLED] = f.w;
            cnt[CHAT_C_UNLABELLED] = f.w == 0;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < CHAT_COUNTERS; ++k) {
        unsigned long long v = cnt[k];
#pragma unroll
        for (int sh = 32; sh; sh >>= 1) v += __shfl_down(v, sh);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&P.counters[k], v);
    }
}

}  // namespace yb
