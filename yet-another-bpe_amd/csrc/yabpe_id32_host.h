// yabpe_id32_host.h -- host driver of the u32-id merge loop (option id_bits = 32).  Included by yabpe.hip
// after its helpers; the kernels are in yabpe_id32_kernels.h.  The entry points of the C ABI branch here when the context's
// id width is 32: set_vocab, the two loads, train, verify_table.  Everything else about a context (options, token bytes,
// stats, the pre-tokeniser, the word pool, encode / decode) is shared.
#pragma once

namespace {

constexpr uint32_t ID32_POOL_MAX = 0xF0000000u;  // token byte pool: offsets are u32

void id32_table_free(PairTable32 &t) {
    dfree(t.keys);
    dfree(t.cnt);
    t.keys = nullptr;
    t.cnt = nullptr;
}

void id32_free_corpus(yabpe_ctx *c) {
    dfree(c->tiles32); dfree(c->tiles32_alt); dfree(c->long_tok32);
    c->tiles32 = c->tiles32_alt = c->long_tok32 = nullptr;
    c->tiles32_alt_cap = 0;
    id32_table_free(c->table32);
}

int id32_table_alloc(yabpe_ctx *c, PairTable32 &t, uint64_t cap, unsigned long long *entries_ctr) {
    uint64_t p2 = 1024;
    while (p2 < cap) p2 <<= 1;
    if (p2 > (1ull << 31)) return fail(c, YABPE_E_CAPACITY, "pair table past 2^31 slots");
    TRY(dmalloc(c, &t.keys, p2));
    TRY(dmalloc(c, &t.cnt, p2));
    t.mask = (uint32_t)(p2 - 1);
    t.max_probe = (uint32_t)std::min<uint64_t>(p2, 2048);
    t.entries = entries_ctr;
    t.cs = nullptr;  // (the candidate list belongs to the main table of a training call: id32_cand_attach)
    t.cand_list = nullptr;
    t.cand_cap = 0;
    HIPCHK(c, hipMemsetAsync(t.keys, 0xFF, p2 * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(t.cnt, 0, p2 * 8, c->stream));
    return 0;
}

Stream32 id32_stream(yabpe_ctx *c) { return Stream32{c->tiles32, c->tile_len, c->tile_wbase, c->wfreq, c->n_tiles}; }
Long32 id32_long(yabpe_ctx *c) { return Long32{c->long_tok32, c->long_off, c->long_len, c->long_freq, c->n_long}; }
uint32_t id32_grid(yabpe_ctx *c) {  // workgroups of a pass over the tile stream: all resident at once
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cdiv64(c->n_tiles, WPB), (uint64_t)std::max(1, c->n_cu) * 4));
}

int id32_count(yabpe_ctx *c, PairTable32 t) {
    if (c->n_tiles) {
        hipLaunchKernelGGL(k32_count, dim3(id32_grid(c)), dim3(BLOCK), 0, c->stream, Count32Params{id32_stream(c), t, c->st});
        HIPCHK(c, hipGetLastError());
    }
    if (c->n_long) {
        hipLaunchKernelGGL(k32_count_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, CountLong32Params{id32_long(c), t, c->st});
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// The candidate list for the main table as it stands now: kept when the table has at least "cand_min_slots" slots (smaller
// tables are scanned whole by every selection), emptied and marked invalid -- the next selection scans the table and lists.
int id32_cand_attach(yabpe_ctx *c) {
    PairTable32 &t = c->table32;
    t.cs = nullptr;
    t.cand_list = nullptr;
    t.cand_cap = 0;
    if (!optv(c, "cand_argmax", 1) || (uint64_t)t.mask + 1 < (uint64_t)std::max<int64_t>(0, optv(c, "cand_min_slots", 1 << 18))) return 0;
    const uint32_t cap = (uint32_t)std::min<int64_t>(1 << 24, std::max<int64_t>(16, optv(c, "cand_cap", 1 << 17)));
    if (!c->cand32_state) {
        TRY(dmalloc(c, &c->cand32_state, 1));
        HIPCHK(c, hipMemsetAsync(c->cand32_state, 0, sizeof(Cand32), c->stream));
        const long long T0 = 1ll << 62;  // (above every count: the first scan finds the best count and sets T from it)
        HIPCHK(c, hipMemcpyAsync(&c->cand32_state->T, &T0, 8, hipMemcpyHostToDevice, c->stream));
    }
    if (c->cand32_cap != cap) {
        dfree(c->cand32_list);
        c->cand32_list = nullptr;
        TRY(dmalloc(c, &c->cand32_list, cap));
        c->cand32_cap = cap;
    }
    HIPCHK(c, hipMemsetAsync(&c->cand32_state->n, 0, 16, c->stream));  // n, overflow, valid, pad
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.cs = c->cand32_state;
    t.cand_list = c->cand32_list;
    t.cand_cap = cap;
    return 0;
}

// a fresh table of at least min_cap slots counted from the stream; grows until no probe sequence ran out and the load is <= 1/2
int id32_table_rebuild(yabpe_ctx *c, uint64_t min_cap) {
    uint64_t cap = std::max<uint64_t>(min_cap, 1024);
    for (int attempt = 0; attempt < 24; ++attempt) {
        id32_table_free(c->table32);
        HIPCHK(c, hipMemsetAsync(&c->st->table_entries, 0, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(&c->st->halt_req, 0, 4, c->stream));
        TRY(id32_table_alloc(c, c->table32, cap, &c->st->table_entries));
        TRY(id32_count(c, c->table32));
        TRY(state_pull(c));
        const uint64_t have = (uint64_t)c->table32.mask + 1;
        if (c->st_host->halt_req == HALT_NONE && c->st_host->table_entries * 2 <= have) {
            c->table_cap = have;
            c->stats.table_rebuilds++;
            return 0;
        }
        cap = have * 2;
    }
    return fail(c, YABPE_E_CAPACITY, "pair table cannot hold the corpus' pairs");
}

// the same pairs in a table of at least new_cap slots (counts of zero are dropped); a recount if a probe sequence runs out
int id32_table_grow(yabpe_ctx *c, uint64_t new_cap) {
    PairTable32 nt{};
    HIPCHK(c, hipMemsetAsync(&c->st->table_entries, 0, 8, c->stream));
    TRY(id32_table_alloc(c, nt, new_cap, &c->st->table_entries));
    const uint64_t old_cap = (uint64_t)c->table32.mask + 1;
    hipLaunchKernelGGL(k32_rehash, dim3((uint32_t)std::min<uint64_t>(1024, cdiv64(old_cap, BLOCK))), dim3(BLOCK), 0, c->stream,
                       Rehash32Params{c->table32, nt, c->st});
    HIPCHK(c, hipGetLastError());
    TRY(state_pull(c));
    id32_table_free(c->table32);
    c->table32 = nt;
    c->table_cap = (uint64_t)nt.mask + 1;
    c->stats.table_rebuilds++;
    if (c->st_host->halt_req != HALT_NONE) return id32_table_rebuild(c, c->table_cap * 2);
    return 0;
}

// ---------------------------------------------------------------------------------------------- vocab
int id32_set_vocab(yabpe_ctx *c, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tokens) {
    if (n_tokens >= YbW32::MAX_TOKENS) return fail(c, YABPE_E_CAPACITY, "base vocabulary too large: ids run 0 .. 2^24 - 3");
    BaseVocab V;
    base_vocab_pack(tok_bytes, tok_off, n_tokens, V);
    // the u32 side: the token-side capacities follow the request (the pool starts at the option and grows, up to
    // ID32_POOL_MAX; the records grow with yabpe_train), rank 0 everywhere -- the u32 selection compares bytes
    uint64_t pool_cap = (uint64_t)optv(c, "pool_bytes", 64 << 20) & ~3ull;
    while (pool_cap < (uint64_t)V.pool.size() + 64) pool_cap = pool_cap * 2 + 64;
    if (pool_cap > ID32_POOL_MAX) return fail(c, YABPE_E_CAPACITY, "base vocabulary bytes exceed the token pool");
    const uint32_t tok_cap = (uint32_t)std::min<uint64_t>(YbW32::MAX_TOKENS, (uint64_t)n_tokens + 4096);
    uint32_t vset_cap = 1u << 14;
    while (vset_cap < 2 * tok_cap) vset_cap <<= 1;
    TRY(base_vocab_index(c, V));
    TRY(base_vocab_upload(c, V, (uint32_t)pool_cap, tok_cap, vset_cap));
    c->tok_cap32 = tok_cap;
    c->pool_growths32 = 0;
    return YABPE_OK;
}

// room for `need` token ids: records, offsets, lengths and the byte-string set (at most half full)
int id32_ensure_tokens(yabpe_ctx *c, uint64_t need) {
    need = std::min<uint64_t>(need, YbW32::MAX_TOKENS);
    if (need <= c->tok_cap32) return 0;
    const uint32_t ncap = (uint32_t)std::min<uint64_t>(YbW32::MAX_TOKENS, std::max<uint64_t>(need, (uint64_t)c->tok_cap32 * 2));
    TRY(state_pull(c));
    const uint32_t n = c->st_host->n_tokens;
    uint32_t *noff = nullptr, *nlen = nullptr;
    TokRec *nrec = nullptr;
    TRY(dmalloc(c, &noff, ncap)); TRY(dmalloc(c, &nlen, ncap)); TRY(dmalloc(c, &nrec, ncap));
    HIPCHK(c, hipMemcpy(noff, c->tt.off, (size_t)n * 4, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(nlen, c->tt.len, (size_t)n * 4, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(nrec, c->tt.rec, (size_t)n * sizeof(TokRec), hipMemcpyDeviceToDevice));
    dfree(c->tt.off); dfree(c->tt.len); dfree(c->tt.rec);
    c->tt.off = noff; c->tt.len = nlen; c->tt.rec = nrec;
    c->tok_cap32 = ncap;
    uint32_t vset_cap = c->tt.vset_mask + 1;
    if (vset_cap < 2 * (uint64_t)ncap) {
        while (vset_cap < 2 * (uint64_t)ncap) vset_cap <<= 1;
        std::vector<TokRec> rec(n);
        HIPCHK(c, hipMemcpy(rec.data(), c->tt.rec, (size_t)n * sizeof(TokRec), hipMemcpyDeviceToHost));
        TRY(upload_vset(c, rec, n, vset_cap));
    }
    c->st_host->tok_len = c->tt.len;  // (the pair table's insert reads the lengths through the state)
    TRY(state_push(c));
    return 0;
}

int id32_grow_pool(yabpe_ctx *c) {
    const uint64_t ncap = std::min<uint64_t>(ID32_POOL_MAX, (uint64_t)c->tt.pool_cap * 2 + 1024) & ~3ull;
    if (ncap <= c->tt.pool_cap) return fail(c, YABPE_E_CAPACITY, "token byte pool exhausted (4 GiB of token bytes)");
    uint8_t *np = nullptr;
    TRY(dmalloc(c, &np, ncap));
    HIPCHK(c, hipMemset(np, 0, ncap));
    HIPCHK(c, hipMemcpy(np, c->tt.pool, c->tt.pool_cap, hipMemcpyDeviceToDevice));
    dfree(c->tt.pool);
    c->tt.pool = np;
    c->tt.pool_cap = (uint32_t)ncap;
    c->pool_growths32++;
    return 0;
}

// ---------------------------------------------------------------------------------------------- corpus
// The u32 load on the load driver's skeleton (LoadRun, the shared steps: yabpe.hip).  What its own two steps hand on:
struct Words32 {
    uint32_t *wtok = nullptr, *wcnt = nullptr, *slots = nullptr, *is_short = nullptr, *is_long = nullptr, *long_len = nullptr;
    unsigned long long *pos = nullptr, *srank = nullptr, *lrank = nullptr, *lpos = nullptr;
    unsigned long long tot[4] = {0, 0, 0, 0};  // slots, short words, long words, long tokens
};

// words as u32 ids (replayed by rp's merges, if any), their places
int id32_load_words(LoadRun &R, const Rp32Table &rp, Words32 &W) {
    yabpe_ctx *c = R.c;
    const LoadInputs &L = R.L;
    const uint64_t n_words = L.n_words;
    Scratch &S = R.S;
    HIPCHK(c, S.get(&W.wtok, L.total_bytes + 1)); HIPCHK(c, S.get(&W.wcnt, n_words + 1));
    HIPCHK(c, S.get(&W.slots, n_words + 1)); HIPCHK(c, S.get(&W.is_short, n_words + 1));
    HIPCHK(c, S.get(&W.is_long, n_words + 1)); HIPCHK(c, S.get(&W.long_len, n_words + 1));
    HIPCHK(c, S.get(&W.pos, n_words + 1)); HIPCHK(c, S.get(&W.srank, n_words + 1));
    HIPCHK(c, S.get(&W.lrank, n_words + 1)); HIPCHK(c, S.get(&W.lpos, n_words + 1));
    HIPCHK(c, hipMemsetAsync(&c->scratch64[1], 0, 16, c->stream));  // [1] frequency overflow, [2] word too long
    if (n_words) {
        const uint32_t wg = cdiv64(n_words, BLOCK);
        hipLaunchKernelGGL(k32_words, dim3(wg), dim3(BLOCK), 0, c->stream,
                           Words32Params{L.bytes, L.off, (unsigned long long)L.off_base, (unsigned long long)n_words, W.wtok, W.wcnt, rp, (uint32_t *)&c->scratch64[2]});
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k32_word_slots, dim3(wg), dim3(BLOCK), 0, c->stream, Slots32Params{W.wcnt, (unsigned long long)n_words, W.slots, W.is_short, W.is_long, W.long_len});
        HIPCHK(c, hipGetLastError());
        const uint32_t *in[4] = {W.slots, W.is_short, W.is_long, W.long_len};
        unsigned long long *out[4] = {W.pos, W.srank, W.lrank, W.lpos};
        for (int k = 0; k < 4; ++k) {
            if (exclusive_scan<uint32_t>(c->stream, in[k], n_words, out[k], (unsigned long long)n_words + 1) != 0)
                return fail(c, YABPE_E_HIP, "scan of the word places failed: %s", hipGetErrorString(hipGetLastError()));
            HIPCHK(c, hipMemcpyAsync(&W.tot[k], out[k] + n_words, 8, hipMemcpyDeviceToHost, c->stream));
        }
        unsigned long long flagsd[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(flagsd, &c->scratch64[1], 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (flagsd[1] & 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a single word longer than 2^32-1 bytes");
    }
    HIPCHK(c, hipEventRecord(R.ev.e[2], c->stream));
    return 0;
}

// the tiles and the long-word buffers sized from the totals and allocated, the words written to them
int id32_load_place(LoadRun &R, const Words32 &W) {
    yabpe_ctx *c = R.c;
    const LoadInputs &L = R.L;
    const uint64_t n_words = L.n_words;
    const unsigned long long *tot = W.tot;
    const uint64_t n_tiles64 = (tot[0] + SPAN32 - 1) / SPAN32;
    if (n_tiles64 >= 0xFFFFFFF0ull || tot[1] >= 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "corpus too large for one context");
    c->n_tiles = (uint32_t)n_tiles64;
    c->n_long = (uint32_t)tot[2];
    c->long_tokens = tot[3];
    c->tiles_cap = c->n_tiles;
    TRY(dmalloc(c, &c->tiles32, (uint64_t)c->n_tiles * CAP32 + 1));
    TRY(dmalloc(c, &c->tile_len, (uint64_t)c->n_tiles + 1));
    TRY(dmalloc(c, &c->tile_wbase, (uint64_t)c->n_tiles + 1));
    TRY(dmalloc(c, &c->wfreq, tot[1] + 1));
    TRY(dmalloc(c, &c->long_tok32, tot[3] + 1));
    TRY(dmalloc(c, &c->long_off, (uint64_t)c->n_long + 1));
    TRY(dmalloc(c, &c->long_len, (uint64_t)c->n_long + 1));
    TRY(dmalloc(c, &c->long_freq, (uint64_t)c->n_long + 1));
    if (n_words) {
        if (c->n_tiles) {
            hipLaunchKernelGGL(k32_build_tiles, dim3(c->n_tiles), dim3(BLOCK), 0, c->stream,
                               Tiles32Params{W.wtok, W.wcnt, L.off, (unsigned long long)L.off_base, (unsigned long long)n_words, W.pos, W.srank, c->tiles32, c->tile_len, c->tile_wbase, c->n_tiles});
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k32_place_words, dim3(cdiv64(n_words, BLOCK)), dim3(BLOCK), 0, c->stream,
                           Place32Params{W.wtok, W.wcnt, L.off, (unsigned long long)L.off_base, (unsigned long long)n_words, L.freq, W.is_short, W.is_long, W.srank, W.lrank, W.lpos,
                                         c->wfreq, c->long_tok32, c->long_off, c->long_len, c->long_freq, (uint32_t *)&c->scratch64[1]});
        HIPCHK(c, hipGetLastError());
        unsigned long long ov = 0;
        HIPCHK(c, hipMemcpyAsync(&ov, &c->scratch64[1], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (ov & 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a word frequency exceeds 2^32-1");
    }
    R.total_tokens = tot[0] - tot[1] + tot[3];
    c->tokens_initial = R.total_tokens;
    // (the u32 load writes resume_stats on every load, the u16 load only on a resumed one)
    c->resume_stats = yabpe_resume_stats_t{};
    c->resume_stats.n_unique = n_words;
    c->resume_stats.tokens = R.total_tokens;
    return 0;
}

// n_merges != 0: a resumed load (the words are rewritten by the model's merges before they are tiled)
int id32_load(yabpe_ctx *c, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words, uint32_t flags,
              const uint32_t *ml, const uint32_t *mr, const uint32_t *mm, uint32_t n_merges) {
    LoadRun R(c);
    TRY(load_check_args(c, word_off, n_words, &R.max_token_bytes));
    if (c->multi) return fail(c, YABPE_E_INVALID, "id_bits = 32 is single-device: this context has a communicator attached");
    Rp32Table rp{{nullptr, nullptr, 0, nullptr}, 0};
    if (n_merges) {  // (checked and built before the loaded corpus is given up; the table lives in R.S until the load returns)
        if (!ml || !mr || !mm) return fail(c, YABPE_E_INVALID, "merge triples are NULL");
        TRY(check_merge_triples(c, ml, mr, mm, n_merges));
        Rp32TableHost th;
        rp_build_table(ml, mr, mm, n_merges, &th);
        TRY(rp_upload<YbW32>(c, R.S, th, &rp));
        rp.n = n_merges;
    }
    id32_free_corpus(c);
    TRY(load_begin(R, bytes, word_off, word_freq, n_words, flags, /*early_release=*/false));  // (the staged inputs stay until the load returns)
    c->weighted = true;  // one layout: a word without a count weighs 1
    Words32 W;
    TRY(id32_load_words(R, rp, W));
    TRY(id32_load_place(R, W));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    R.In.release(); R.S.release();
    TRY(load_state_reset(c, R.total_tokens, R.max_token_bytes, &W.tot[0]));  // (live_slots: the scan's total; u16 sums tile_len)
    // (its own table builder, at the table_min_log2 size; the u16 load starts at 2^18 slots)
    TRY(id32_table_rebuild(c, (uint64_t)1 << std::min<int64_t>(30, std::max<int64_t>(10, optv(c, "table_min_log2", 16)))));
    // (its job_reset also resets the exchange's counters and blk_read: id_bits is fixed and this load refuses a communicator -- unobservable)
    return load_account(R, /*replayed=*/true);
}

// ---------------------------------------------------------------------------------------------- repack
// The live slots packed again word by word into ceil(live / SPAN32) tiles (k32_repack: plan, then move).
int id32_repack(yabpe_ctx *c) {
    const uint32_t n = c->n_tiles;
    Scratch S(c->device, c->rank);
    unsigned long long *d_base = nullptr, *d_first = nullptr;
    HIPCHK(c, S.get(&d_base, (uint64_t)n + 1));
    if (exclusive_scan<uint32_t>(c->stream, c->tile_len, n, d_base, (unsigned long long)n + 1) != 0)
        return fail(c, YABPE_E_HIP, "scan of the tile lengths failed: %s", hipGetErrorString(hipGetLastError()));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_base + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t n_new = (uint32_t)((total + SPAN32 - 1) / SPAN32);
    if (n_new >= n || n_new == 0) return 0;
    uint32_t *nlen = nullptr, *nwb = nullptr;
    if (c->tiles32_alt_cap < n_new) {
        dfree(c->tiles32_alt);
        c->tiles32_alt = nullptr;
        c->tiles32_alt_cap = 0;
        TRY(dmalloc(c, &c->tiles32_alt, (uint64_t)n_new * CAP32 + 1));
        c->tiles32_alt_cap = n_new;
    }
    HIPCHK(c, S.get(&d_first, (uint64_t)n_new + 1));
    TRY(dmalloc(c, &nlen, (uint64_t)n_new + 1));
    TRY(dmalloc(c, &nwb, (uint64_t)n_new + 1));
    HIPCHK(c, hipMemsetAsync(d_first, 0xFF, ((size_t)n_new + 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(nwb, 0xFF, ((size_t)n_new + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(nlen, 0, ((size_t)n_new + 1) * 4, c->stream));
    const Repack32Params P{id32_stream(c), d_base, d_first, c->tiles32_alt, nlen, nwb, n_new};
    hipLaunchKernelGGL(k32_repack<false>, dim3(id32_grid(c)), dim3(BLOCK), 0, c->stream, P);
    hipLaunchKernelGGL(k32_repack<true>, dim3(id32_grid(c)), dim3(BLOCK), 0, c->stream, P);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(c->tiles32, c->tiles32_alt);
    std::swap(c->tiles_cap, c->tiles32_alt_cap);
    dfree(c->tile_len); dfree(c->tile_wbase);
    c->tile_len = nlen;
    c->tile_wbase = nwb;
    c->n_tiles = n_new;
    c->stats.retiles++;
    return 0;
}

int id32_refresh_live(yabpe_ctx *c) {
    HIPCHK(c, hipMemsetAsync(&c->scratch64[0], 0, 8, c->stream));
    if (c->n_tiles) {
        hipLaunchKernelGGL(k32_sum_len, dim3((uint32_t)std::min<uint64_t>(1024, cdiv64(c->n_tiles, BLOCK))), dim3(BLOCK), 0, c->stream, c->tile_len, c->n_tiles, &c->scratch64[0]);
        HIPCHK(c, hipGetLastError());
    }
    unsigned long long v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, &c->scratch64[0], 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->st_host->live_slots = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------- verify
int id32_verify(yabpe_ctx *c, uint64_t *out_mismatches) {
    PairTable32 scratch{};
    HIPCHK(c, hipMemsetAsync(&c->scratch64[4], 0, 16, c->stream));  // [4] entries, [5] mismatches
    TRY(id32_table_alloc(c, scratch, (uint64_t)c->table32.mask + 1, &c->scratch64[4]));
    scratch.max_probe = scratch.mask + 1;  // (the recount must not give up where the main table did not)
    TRY(id32_count(c, scratch));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, cdiv64((uint64_t)scratch.mask + 1, BLOCK));
    hipLaunchKernelGGL(k32_table_compare, dim3(grid), dim3(BLOCK), 0, c->stream, Compare32Params{c->table32, scratch, &c->scratch64[5], 0u});
    hipLaunchKernelGGL(k32_table_compare, dim3(grid), dim3(BLOCK), 0, c->stream, Compare32Params{scratch, c->table32, &c->scratch64[5], 1u});
    HIPCHK(c, hipGetLastError());
    unsigned long long mm = 0;
    HIPCHK(c, hipMemcpyAsync(&mm, &c->scratch64[5], 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    id32_table_free(scratch);
    HIPCHK(c, hipMemsetAsync(&c->st->halt_req, 0, 4, c->stream));
    *out_mismatches = mm;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- train
int id32_train(yabpe_ctx *c, uint32_t num_merges, uint64_t min_frequency, uint32_t *out_left, uint32_t *out_right, uint32_t *out_merged,
               uint64_t *out_count, uint32_t *out_n_merges) {
    uint32_t rec_base = 0;
    TRY(train_begin(c, num_merges, min_frequency, &rec_base));
    DevState *h = c->st_host;
    if (num_merges == 0) return YABPE_OK;
    // token-side capacities follow the request (every merge may take an id), the per-merge records too: all of them at
    // once, where the u16 loop starts with its id space's worth and grows
    TRY(id32_ensure_tokens(c, (uint64_t)h->n_tokens + num_merges));
    TRY(train_begin_records(c, num_merges));
    if (!c->sel_ticket) {
        TRY(dmalloc(c, &c->sel_ticket, TICKET_WORDS));
        HIPCHK(c, hipMemsetAsync(c->sel_ticket, 0, TICKET_WORDS * 4, c->stream));
    }
    if (!c->partials32) TRY(dmalloc(c, &c->partials32, SEL32_MAX_BLOCKS));
    const uint32_t check = (uint32_t)std::max<int64_t>(1, optv(c, "check_interval", 32));
    const int64_t retile_pct = optv(c, "retile_pct", 60), table_load_pct = optv(c, "table_load_pct", 30);
    const uint64_t retile_min_tiles = (uint64_t)std::max<int64_t>(2, optv(c, "retile_min_tiles", 4096));
    const uint32_t id_limit = (uint32_t)std::min<int64_t>(YbW32::MAX_TOKENS, std::max<int64_t>(256, optv(c, "id32_limit", YbW32::MAX_TOKENS)));
    Events<2> T;  // start, end
    HIPCHK(c, T.create());
    HIPCHK(c, hipEventRecord(T.e[0], c->stream));
    uint64_t stream_bytes = 0, launches = 0;
    TRY(id32_cand_attach(c));
    uint32_t idle_rounds = 0;
    for (;;) {
        // one round: `check` merges, each a selection and an apply pass; kernels of a finished or halted job return at once
        const uint64_t cap = (uint64_t)c->table32.mask + 1;
        const uint32_t sel_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(SEL32_MAX_BLOCKS, cap / (BLOCK * 16)));
        const Select32Params SP{c->table32, c->tt, c->st, c->partials32, c->sel_ticket, c->rec_left, c->rec_right, c->rec_merged, c->rec_count,
                                rec_base, c->tok_cap32, id_limit};
        const Apply32Params AP{id32_stream(c), c->table32, c->st, c->rec_sites, rec_base};
        const ApplyLong32Params LP{id32_long(c), c->table32, c->st, c->rec_sites, rec_base};
        const uint32_t left = num_merges - (h->iter - rec_base);
        const uint32_t round = std::min(check, left + 1);  // (+ 1: the selection that sees the limit and sets done)
        for (uint32_t k = 0; k < round; ++k) {
            hipLaunchKernelGGL(k32_select, dim3(sel_grid), dim3(BLOCK), 0, c->stream, SP);
            if (c->n_tiles) hipLaunchKernelGGL(k32_apply, dim3(id32_grid(c)), dim3(BLOCK), 0, c->stream, AP);
            if (c->n_long) hipLaunchKernelGGL(k32_apply_long, dim3(cdiv64(c->n_long, 64)), dim3(64), 0, c->stream, LP);
        }
        HIPCHK(c, hipGetLastError());
        const uint32_t before = h->iter;
        TRY(state_pull(c));
        // (a selection whose candidate list drained commits nothing; the one after it scans the whole table and does)
        idle_rounds = (h->iter == before && h->halt == HALT_NONE && !h->done) ? idle_rounds + 1 : 0;
        if (idle_rounds >= 4) return fail(c, YABPE_E_INTERNAL, "the selection made no progress after %u merges", h->iter - rec_base);
        launches += h->iter - before;
        stream_bytes += (uint64_t)(h->iter - before) * (h->live_slots * 4 + (uint64_t)c->n_tiles * 8);
        if (h->halt != HALT_NONE) {
            const uint32_t why = h->halt;
            if (why == HALT_VOCAB_FULL) {
                if (h->n_tokens >= id_limit) return fail(c, YABPE_E_CAPACITY, "u32 token id space exhausted (ids run 0 .. 2^24 - 3) after %u merges", h->iter - rec_base);
                TRY(id32_ensure_tokens(c, (uint64_t)h->n_tokens + (num_merges - (h->iter - rec_base))));
                TRY(state_pull(c));
            } else if (why == HALT_POOL_FULL) {
                TRY(id32_grow_pool(c));
            } else if (why == HALT_TABLE_FULL) {
                // a probe sequence ran out during an apply pass: its deltas are lost, the stream is whole -- a larger table, recounted
                TRY(id32_table_rebuild(c, ((uint64_t)c->table32.mask + 1) * 2));
                TRY(id32_cand_attach(c));
                TRY(state_pull(c));
            } else {
                return fail(c, YABPE_E_INTERNAL, "device halt %u after %u merges", why, h->iter - rec_base);
            }
            h->halt = HALT_NONE;
            h->halt_req = HALT_NONE;
            TRY(state_push(c));
            continue;
        }
        if (h->done || h->iter - rec_base >= num_merges) {
            // (the last committed merge has been applied: every selection is followed by its apply pass)
            if (h->halt_req == HALT_TABLE_FULL) {
                TRY(id32_table_rebuild(c, ((uint64_t)c->table32.mask + 1) * 2));
                TRY(state_pull(c));
                h->halt_req = HALT_NONE;
                TRY(state_push(c));
            }
            break;
        }
        if (table_grow_rule(h->table_entries, (uint64_t)c->table32.mask + 1, table_load_pct)) {  // (the u16 loop's load rule; the target is this loop's own)
            TRY(id32_table_grow(c, table_grow_target_rule(h->table_entries, 4, 1024)));
            TRY(id32_cand_attach(c));
            TRY(state_pull(c));
        }
        TRY(id32_refresh_live(c));
        TRY(state_push(c));
        if (retile_rule(c->n_tiles, retile_min_tiles, h->live_slots, retile_pct, SPAN32)) TRY(id32_repack(c));
    }
    HIPCHK(c, hipEventRecord(T.e[1], c->stream));
    HIPCHK(c, hipEventSynchronize(T.e[1]));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, T.e[0], T.e[1]));
    c->stats.train_ms += ms;
    if (c->table32.cs) {  // scans of the whole table that (re)built the list; selections that found it drained
        Cand32 hs{};
        HIPCHK(c, hipMemcpy(&hs, c->cand32_state, sizeof hs, hipMemcpyDeviceToHost));
        c->cand_rebuilds = hs.rebuilds;
        c->cand_rescans = hs.drains;
    }
    c->table32.cs = nullptr;  // (verify, rehash and recount see a plain table; the next call attaches the list again)
    c->stats.dense_launches += launches;
    c->stats.dense_merges += launches;
    c->stats.dense_actual_bytes_sampled += stream_bytes;  // (every launch counted: bytes of live slots + tile lengths read)
    TRY(state_pull(c));
    h->tokens_now -= h->sites;
    h->sites = 0;
    TRY(state_push(c));
    TRY(train_copy_out(c, h->iter - rec_base, false, out_left, out_right, out_merged, out_count, out_n_merges));  // (no live-slot log: rec_live is the u16 selection's)
    if (optv(c, "verify", 0)) {
        uint64_t mm = 0;
        TRY(id32_verify(c, &mm));
        if (mm) return fail(c, YABPE_E_INTERNAL, "incremental pair table differs from a recount in %llu keys", (unsigned long long)mm);
    }
    return YABPE_OK;
}

}  // namespace
