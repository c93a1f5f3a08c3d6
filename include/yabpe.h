/*
 * yabpe.h -- C ABI of the MI355X-native BPE training hot path (libyabpe.so).
 *
 * The reference (DreamOneX/yet-another-bpe) is pure Python and has no FFI: its seam for this path is the
 * method BBPETrainer._merge_loop (src/yet_another_bpe/trainer.py:216-302), fed by train() (:63-92).
 * These entry points are what a binding for that method needs; each one names the reference lines whose
 * RESULT it reproduces.  Plain pointers and sizes only (no torch / numpy types); every pointer the caller
 * passes stays owned by the caller; the library owns only its opaque context and the device buffers it
 * hands out through yabpe_synth_generate().
 *
 * All functions return 0 (YABPE_OK) or a negative error code; yabpe_last_error() gives the message.
 * A context is bound to one GPU and must not be used from two threads at once.
 * There is NO CPU fallback: without a usable gfx950 device yabpe_create() fails with YABPE_E_NODEVICE.
 */
#ifndef YABPE_H
#define YABPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YABPE_ABI_VERSION 2

enum {
    YABPE_OK = 0,
    YABPE_E_INVALID = -1,  /* bad argument / call order */
    YABPE_E_NODEVICE = -2, /* no HIP device */
    YABPE_E_HIP = -3,      /* HIP runtime error (message has the call) */
    YABPE_E_CAPACITY = -4, /* a documented limit was hit (token ids: at most 65534 tokens with id_bits = 16, 2^24 - 2 with 32) */
    YABPE_E_INTERNAL = -5, /* device-side invariant violated */
    YABPE_E_COMM = -6,     /* RCCL error */
    YABPE_E_UTF8 = -7      /* yabpe_pretokenize: the text is not valid UTF-8 (position reported) */
};

/* yabpe_load_words flags */
#define YABPE_LOAD_DEDUP 0x1u /* pool equal words on the device first (trainer.py:221-225) */

typedef struct yabpe_ctx yabpe_ctx;

/* Library / device ---------------------------------------------------------------------------------- */
int yabpe_abi_version(void);
int yabpe_device_count(void);

/* Creates a context on HIP device `device_id`.  One context per _merge_loop call (or reuse via yabpe_reset). */
int yabpe_create(yabpe_ctx **out, int device_id);
void yabpe_destroy(yabpe_ctx *ctx);
/* Message of the last error on this context (ctx == NULL: of the last failed yabpe_create). Never NULL. */
const char *yabpe_last_error(const yabpe_ctx *ctx);

/* Tunables by name (see DESIGN.md "Tunables"): "check_interval", "retile_pct", "apply_blocks", "event_sample",
   "table_min_log2", "skip_index", "cand_argmax", "verify" ... */
int yabpe_set_option(yabpe_ctx *ctx, const char *name, int64_t value);
/* Option "id_bits": the id width of the merge loop, 16 (the default) or 32; anything else: YABPE_E_INVALID.  Read by
 * yabpe_set_vocab and fixed from then on: setting another value afterwards is YABPE_E_INVALID (the value it has is accepted).
 * With 16 every call is what it always was: ids 0 .. 65,533, and a job that needs one more id ends in YABPE_E_CAPACITY.
 * With 32 ids run 0 .. 2^24 - 3 (the bound of yabpe_decode_set_model's table, so a trained model can always be
 * decoded on the device); past it yabpe_train returns YABPE_E_CAPACITY as before.  The token stream is u32 with 32-bit SEP /
 * PAD, the pair key a u64 (left << 24 | right), the token-side capacities follow the request.  One layout, the pooled one: a
 * load without word_freq and without YABPE_LOAD_DEDUP gives every word the weight 1 -- the same arithmetic and the same
 * model; yabpe_load_words_resumed, "max_token_bytes", word_freq up to 2^32 - 1 and long words work as they do at 16 bits.  One
 * form: one merge per launch over the whole live stream, the selection a launch of its own.  yabpe_n_tokens,
 * yabpe_token_bytes, yabpe_stats (its pool_growths counts the growths of the token byte pool), yabpe_resume_stats and
 * yabpe_verify_table serve both widths.  Refused with YABPE_E_INVALID and a message: yabpe_stream_dump and
 * yabpe_stream_checksum (their slots are u16), and every communicator (yabpe_comm_init / yabpe_comm_init_custom on a context
 * with id_bits = 32, or id_bits = 32 on a context that has one): training with u32 ids is single-device. */

/* Base vocabulary ------------------------------------------------------------------------------------
 * Result of _init_base_vocab (trainer.py:119-134): ids 0..n_tokens-1, token i = tok_bytes[tok_off[i]..tok_off[i+1]).
 * The first 256 entries must be the single bytes 0..255 in order (trainer.py:123-125).  The host computes the
 * list (dedup rule of :130 included); the device needs the bytes for the byte-lexicographic tie-break (:246)
 * and for "merged not in vocab" (:298). */
int yabpe_set_vocab(yabpe_ctx *ctx, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tokens);

/* Corpus ---------------------------------------------------------------------------------------------
 * The `sequences` argument of _merge_loop (trainer.py:216) as flat buffers: word i = bytes[word_off[i]..word_off[i+1]).
 * word_freq == NULL means every word counts once (flat layout: every occurrence resident in HBM).
 * With word_freq the caller has already pooled equal words (trainer.py:221-225) and passes their counts.
 * Pointers may be host or device memory (detected); device buffers are read in place, host buffers are staged. */
int yabpe_load_words(yabpe_ctx *ctx, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq,
                     uint64_t n_words, uint32_t flags);

/* Continuing from a trained model: the same corpus arguments as yabpe_load_words, plus the model's merges as id triples in
 * order (left, right, merged: what replaying model.merges over the base vocabulary as _decode_merges does gives).  Call after
 * yabpe_set_vocab with ALL of the model's tokens in id order.  Every word is brought to the state the training loop would
 * have left it in -- rewritten by merge 0, then merge 1, ... each over its id pair, greedily from the left -- and tiled by
 * its token count; yabpe_train then continues (new merges get the next ids).  Needs the pooled layout (word_freq or
 * YABPE_LOAD_DEDUP), else YABPE_E_INVALID; a triple that names an id >= n_tokens or whose merged token is not as long as
 * its operands together: YABPE_E_INVALID.  n_merges == 0 behaves as yabpe_load_words.  Single GPU. */
int yabpe_load_words_resumed(yabpe_ctx *ctx, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq,
                             uint64_t n_words, uint32_t flags, const uint32_t *merge_left, const uint32_t *merge_right,
                             const uint32_t *merge_merged, uint32_t n_merges);
/* What the last resumed load saw (HIP events; segment_ms includes the pooling of equal words, build_ms the tiles and the
 * initial pair count). */
typedef struct yabpe_resume_stats_t {
    uint64_t n_unique;   /* pooled words */
    uint64_t n_long;     /* ... of them long by their TOKEN count after the replay */
    uint64_t tokens;     /* tokens after the replay */
    double segment_ms;
    double build_ms;
} yabpe_resume_stats_t;
int yabpe_resume_stats(yabpe_ctx *ctx, yabpe_resume_stats_t *out);

/* Merge loop -----------------------------------------------------------------------------------------
 * Runs trainer.py:238-300: at most `num_merges` iterations (the host computes max(0, vocab_size - len(vocab)),
 * :238), stops early when no pair is left (:242-243) or the best count < min_frequency (:247-248).
 * Outputs, one entry per merge in selection order (arrays of capacity num_merges, may be NULL):
 *   out_left/out_right   ids of the merged pair            (merges.append(best_pair), :296)
 *   out_merged           id of left+right: a fresh id, or the existing id when those bytes are already a
 *                        token (no id consumed, :298-300)
 *   out_count            the pair's count when it was selected
 * May be called again to continue training with more merges.
 *
 * Maximum token length: option "max_token_bytes" (yabpe_set_option; 0, the default: no limit; N >= 2: the limit in bytes).
 * With a limit the best pair of every step is the maximum over the pairs whose two tokens are together at most N bytes
 * long, and the stop rules look at that pair: training stops when no such pair is left or its count is below
 * min_frequency, whatever longer pairs count.  Everything else is unchanged; base-vocabulary tokens (specials) and the
 * merges a resumed load replays are not subject to it.  The limit is a property of a LOAD, not of a yabpe_train call: it is
 * read by yabpe_load_words / yabpe_load_words_resumed and holds until the next load -- for every yabpe_train call on that
 * load and for yabpe_verify_table; setting the option later changes nothing until words are loaded again.  (Pairs over the
 * limit are never put into the pair table, so one dropped under a tight limit could not be recovered by loosening it, and
 * one admitted under a loose limit would survive tightening.)  1 or a negative value: YABPE_E_INVALID from the next load. */
int yabpe_train(yabpe_ctx *ctx, uint32_t num_merges, uint64_t min_frequency, uint32_t *out_left,
                uint32_t *out_right, uint32_t *out_merged, uint64_t *out_count, uint32_t *out_n_merges);

/* Token bytes after training: token id -> bytes (vocab of trainer.py:302, inverted). */
int yabpe_n_tokens(yabpe_ctx *ctx, uint32_t *out_n_tokens);
int yabpe_token_bytes(yabpe_ctx *ctx, uint32_t id, uint8_t *out, uint32_t cap, uint32_t *out_len);

/* Measurement ---------------------------------------------------------------------------------------- */
typedef struct yabpe_stats_t {
    uint64_t n_words;          /* W: resident words (after optional dedup) */
    uint64_t n_words_input;    /* words passed to yabpe_load_words */
    uint64_t n_long_words;     /* words handled by the long-word path */
    uint64_t tokens_initial;   /* T_0 */
    uint64_t tokens_now;       /* T_i = T_0 - sum of merged sites */
    uint64_t merges_done;
    uint64_t n_tiles;
    uint64_t live_slots;       /* u16 slots the apply kernel currently reads */
    uint64_t table_capacity;
    uint64_t table_entries;
    uint64_t retiles, table_rebuilds;
    double load_ms;            /* yabpe_load_words device time */
    double train_ms;           /* device time of all yabpe_train calls (event-timed) */
    double apply_ms_sampled;   /* sum of the event-timed apply phases (k_apply, or k_scan + k_slow) */
    uint64_t apply_launches_sampled;
    uint64_t apply_algo_bytes_sampled;   /* sum of 2*(T_i + W) over the sampled launches */
    uint64_t apply_actual_bytes_sampled; /* sum of 2*live_slots over the sampled launches */
    uint64_t algo_bytes_total;           /* sum over all iterations of 2*(T_i + W) */
    /* split form only: the streaming scan kernel (k_scan) by itself */
    double scan_ms_sampled;
    uint64_t scan_launches_sampled;
    uint64_t scan_algo_bytes_sampled;
    uint64_t scan_actual_bytes_sampled;
    /* skip index: launches of k_scan_skip and the tiles they actually read (the rest was skipped by signature) */
    uint64_t scan_skip_launches;
    uint64_t scan_skip_tiles_read;
    /* candidate argmax: rebuilds of the candidate list (scans of the table) and batches that fell back to the full table scan */
    uint64_t cand_rebuilds;
    uint64_t cand_rescans;
    /* fused per-merge launches: apply of merge i + selection of merge i+1 in one kernel (the production form) */
    uint64_t fused_launches;
    /* the streaming phase: event-timed launches of the fused k_apply (whole iteration when the selection is fused in) */
    double dense_ms_sampled;
    uint64_t dense_launches_sampled;
    uint64_t dense_algo_bytes_sampled;   /* sum of 2*(T_i + W) over them */
    uint64_t dense_actual_bytes_sampled; /* sum of the bytes of live slots + tile lengths they read */
    /* the sparse phase (skip index): device time from the switch to the end of the last yabpe_train call, merges applied in it */
    double sparse_ms;
    uint64_t sparse_merges;
    /* the second half of each yabpe_train call's merges (few sites per merge: the latency-bound regime) */
    double tail_ms;
    uint64_t tail_merges;
    /* multi-GPU: all-gathers of [header | records] buffers (one per merge), bytes every rank receives per exchange, record
       capacity per rank, times the buffers had to grow (a merge produced more records than fit: global recount) */
    uint64_t exchanges, exchange_bytes, exchange_cap_records, exchange_growths, exchange_max_records;
    /* launches of the sparse phase: one launch applies a BATCH of merges (sparse_merges / sparse_launches = mean batch) */
    uint64_t sparse_launches;
    /* ... and the launches of the second half of each yabpe_train call's merges (tail_merges / tail_launches = mean batch there) */
    uint64_t tail_launches;
    /* peer-to-peer exchange: device time of the event-timed push-and-wait launches (one per round of launches) */
    double exchange_ms_sampled;
    uint64_t exchanges_sampled;
    uint64_t exchange_p2p;     /* 1: the exchanges go peer to peer (0: through the attached transport's all-gather) */
    /* the streaming phase: its launches and the merges they applied (a launch applies a batch of up to "batch_max_stream"
       merges in one pass over the stream); dense_algo_bytes_sampled / dense_actual_bytes_sampled are the phase's totals
       scaled to the event-timed launches */
    uint64_t dense_launches, dense_merges;
    /* sparse launches over a stream of more chunks than workgroups: pieces of the second round taken from the shared counter */
    uint64_t scan_skip_pieces_taken;
    /* id_bits = 32: times the token byte pool (option "pool_bytes": its first size) had to grow */
    uint64_t pool_growths;
} yabpe_stats_t;
int yabpe_stats(yabpe_ctx *ctx, yabpe_stats_t *out);
/* Per-iteration log of the last yabpe_train call: sites merged M_i and live slots read by iteration i. */
int yabpe_iter_log(yabpe_ctx *ctx, uint64_t *out_sites, uint64_t *out_live_slots, uint32_t cap, uint32_t *out_n);

/* Per-launch HIP-event timings of k_apply from the last yabpe_train call (option "event_sample" = N times every
   Nth launch): iteration index (relative to the call), duration of the whole apply phase and of its streaming
   kernel (k_scan / k_scan_skip, or the fused k_apply) in microseconds. */
int yabpe_event_log(yabpe_ctx *ctx, uint32_t *out_iter, float *out_us, float *out_scan_us, uint32_t cap, uint32_t *out_n);

/* Latency pieces of one sparse merge, measured on the (otherwise idle) device: what the floor of the per-merge launch is
   built from (bench.py prints the model).  All in microseconds. */
typedef struct yabpe_latency_t {
    double launch_gap_us;       /* back-to-back dependent launches of an empty kernel on one stream, per launch */
    double load_trip_us;        /* one dependent global load that misses the caches (pointer chase, one lane) */
    double coherent_trip_us;    /* the same with device-scope loads (hand-offs inside a launch) */
    double atomic_trip_us;      /* one dependent returning device-scope atomic */
} yabpe_latency_t;
int yabpe_latency_probe(yabpe_ctx *ctx, yabpe_latency_t *out);

/* Debug / self-check: recount every pair from the token stream into a scratch table and compare with the
   incrementally maintained table.  *out_mismatches = number of differing keys. */
int yabpe_verify_table(yabpe_ctx *ctx, uint64_t *out_mismatches);
/* Debug: decode the resident token stream back to bytes and return an order-independent checksum over
   (word bytes, segmentation) plus the number of words/tokens it saw (the long-word buffer included). */
int yabpe_stream_checksum(yabpe_ctx *ctx, uint64_t *out_sum, uint64_t *out_words, uint64_t *out_tokens);
/* Debug: copy the resident tile stream to the host as it lies in memory (the checksum above is order-independent and cannot
   see where a word was placed).  *out_n_tiles and *out_flags are always written; call once with NULL buffers to size them.
   Every buffer may be NULL: tiles 1024 u16 slots per tile, tile_len and tile_wbase one u32 per tile (tile_wbase only with
   YABPE_DUMP_WBASE: the layout with frequencies), sig 512 rows of n_tiles u64 (only with YABPE_DUMP_SIG: the skip index is valid). */
#define YABPE_DUMP_WBASE 0x1u
#define YABPE_DUMP_SIG 0x2u
int yabpe_stream_dump(yabpe_ctx *ctx, uint32_t *out_n_tiles, uint32_t *out_flags, uint16_t *tiles, uint32_t *tile_len,
                      uint32_t *tile_wbase, uint64_t *sig);

/* Synthetic corpus of SURVEY.md 8(d), generated on the device (bit-identical to yet_another_bpe/synth.py).
   Returns device pointers owned by the library (freed by yabpe_synth_free or yabpe_destroy). */
int yabpe_synth_generate(yabpe_ctx *ctx, uint64_t target_bytes, uint32_t n_types, uint64_t seed,
                         const uint8_t *alphabet, uint32_t alphabet_len, int space_prefix,
                         uint8_t **out_dev_bytes, uint64_t **out_dev_off, uint64_t *out_n_words, uint64_t *out_n_bytes);
/* The same Zipf draw (w_j = floor(2^40 / (j+1)), u = rnd(seed,3,i) % sum w) over a lexicon the caller supplies (host arrays:
   bytes + n_types+1 offsets, every entry 1..65,535 bytes): the drawn entries are concatenated until target_bytes is reached.
   For synthetic TEXT (yet_another_bpe/synth.py text_lexicon: multi-byte UTF-8 words, digits, punctuation, whitespace runs,
   long letter runs) whose pre-tokens yabpe_pretokenize then finds; out_dev_off are the piece boundaries (not pre-tokens). */
int yabpe_synth_generate_lex(yabpe_ctx *ctx, uint64_t target_bytes, uint32_t n_types, uint64_t seed,
                             const uint8_t *lex_bytes, const uint64_t *lex_off,
                             uint8_t **out_dev_bytes, uint64_t **out_dev_off, uint64_t *out_n_pieces, uint64_t *out_n_bytes);
int yabpe_synth_free(yabpe_ctx *ctx);
/* Copy `n` bytes device->host / host->device (for fixtures and the CPU-baseline sample). */
int yabpe_memcpy_d2h(yabpe_ctx *ctx, void *dst_host, const void *src_dev, uint64_t n);
int yabpe_memcpy_h2d(yabpe_ctx *ctx, void *dst_dev, const void *src_host, uint64_t n);

/* Pre-tokeniser (the step before the path) -----------------------------------------
 * Reproduces _preprocess_corpus (trainer.py:136-214) on the device: every chunk [chunk_off[k], chunk_off[k+1]) of `text`
 * (the last one ends at n_bytes; chunk_off == NULL: one chunk) is decoded as UTF-8 and split with the GPT-2 pattern of
 * trainer.py:163, preceded by the special tokens in the given order (:165-167), exactly as regex.findall does.  The host
 * keeps what it does in the reference: reading files and choosing the chunk cuts (:172-198).
 * Results: *out_dev_text = the text in device memory (`text` itself when it already is a device pointer, else a staged
 * copy owned by the library) and *out_dev_word_off = n_words + 1 offsets into it (device memory, owned by the library,
 * released by yabpe_pretokenize_free / yabpe_destroy): pre-token i = text[off[i], off[i+1]).  Both can be passed
 * straight to yabpe_load_words (no copy; add YABPE_LOAD_DEDUP to pool equal pre-tokens, trainer.py:221-225).
 * Malformed UTF-8: returns YABPE_E_UTF8 and *out_bad_pos = UnicodeDecodeError.start of the first bad chunk (:156-161).
 * The character classes (\p{L}, \p{N}, \s) are those of the third-party `regex` module the reference uses
 * (csrc/unicode_classes.inc, generated by tools/gen_unicode_classes.py).
 * Digit groups: option "digit_group" (yabpe_set_option; 0, the default: the GPT-2 pattern as it is; G in 1 .. 255: \p{N}+ is
 * replaced by \p{N}{1,G}, the digit rule of the GPT-4 / Llama-3 family (G = 3) and of the single-digit family (G = 1)).  The
 * option is read by every yabpe_pretokenize, yabpe_encode, yabpe_encode_spans and yabpe_encode_dropout call; any other value
 * makes that call return YABPE_E_INVALID.  The rule, on the starts the GPT-2 pattern gives (specials included): in every
 * pre-token that is a run of \p{N} characters (with or without the U+0020 in front) the characters are numbered 0, 1, 2, ..
 * from the first digit, and a new pre-token starts at every one whose number is a positive multiple of G.  Characters are
 * counted, not bytes; a chunk start and the end of a special start a new run.  With G >= 1 a special token whose first
 * character is \p{N} is rejected (YABPE_E_INVALID, the message names it): it could match at a group boundary, where the
 * GPT-2 pattern has no token start.  The pass costs three more kernels (linear in the text whatever it holds, a file of
 * digits included); with 0 nothing is launched or allocated for it.
 * Split pattern: option "split_pattern" (yabpe_set_option; 0, the default: the GPT-2 pattern; 1: the cl100k pattern of GPT-4,
 * Llama-3 (digit_group 3) and Qwen2 (digit_group 1),
 *   (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,G}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * with G = the option "digit_group", which must then be 1 .. 255).  Read by the same four calls; any value but 0, 1 and 3 (below), or 1
 * with digit_group 0, makes the call return YABPE_E_INVALID.  Against GPT-2: contractions match in either case; one character that
 * is no letter, digit, CR or LF joins the letter run behind it; digits take no space in front; a run of punctuation swallows
 * the CR / LF behind it, and a whitespace run that holds a CR / LF is cut after its last one (csrc/split4_logic.h has the
 * rule per position).  With 1 a special token of yabpe_pretokenize whose first character is \s or \p{N} is rejected
 * (YABPE_E_INVALID, the message names it): whether a token starts at a whitespace character can depend on the whole
 * whitespace run, which is known only after the specials are placed.  The newline rules cost three more kernels in front of
 * the digit groups (two segmented scans, linear on a file of blank lines or a newline and a gigabyte of spaces); with 0
 * nothing of this is launched or allocated, and the GPT-2 kernels are the ones that run.
 * 3: the o200k_base pattern of GPT-4o, the o-series and gpt-oss (2 is reserved and refused),
 *   [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *   |[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *   |\p{N}{1,G}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * again with G = "digit_group" in 1 .. 255 (3 with digit_group 0: YABPE_E_INVALID).  Against cl100k: a word is cut where its
 * case changes (HTTPServer | " foo" | Bar), the contraction stays with its word, \p{M} counts as a letter inside a word, and
 * "/" is kept behind the newlines that follow punctuation.  No rule of it has bounded reach, so the device runs it as a
 * scanner of 13 states: classes, one backward scan of two look-ahead bits, one forward scan of state-transition functions
 * (csrc/split5_logic.h; nine kernels in place of the fused pass, one more array of n_bytes, linear on any text).  With 3 a
 * special token of yabpe_pretokenize is taken wherever the scanner stands at a token boundary at its first byte, so
 * occurrences must never overlap: rejected (YABPE_E_INVALID, the message names the specials) are a special that contains
 * another one, a special one of whose proper suffixes begins a special (itself included; equal specials count as one), and,
 * as with 1, a special whose first character is \s or \p{N}.  "<|endoftext|>", "<|im_start|>" and "<|im_end|>" pass. */
int yabpe_pretokenize(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off, uint32_t n_chunks,
                      const uint8_t *special_bytes, const uint32_t *special_off, uint32_t n_special,
                      const uint8_t **out_dev_text, uint64_t **out_dev_word_off, uint64_t *out_n_words, int64_t *out_bad_pos);
int yabpe_pretokenize_free(yabpe_ctx *ctx);

/* Normaliser (the step in front of the pre-tokeniser and of the encoder) ---------------------------------
 * Unicode NFC on the device: every part [part_off[k], part_off[k+1]) of `text` (the last one ends at n_bytes; part_off == NULL:
 * one part; read as yabpe_pretokenize reads chunk_off: n_parts ascending starts, the first one 0) is replaced by
 * unicodedata.normalize("NFC", part) of CPython, Unicode version as csrc/unicode_norm.inc says (generated by
 * tools/gen_unicode_norm.py from the installed unicodedata).  Parts are normalised independently: a part that begins with a
 * combining mark does not combine with the part before it.  form: YABPE_NORM_NFC; anything else: YABPE_E_INVALID.
 * text may be host or device memory.  Results (owned by the library, valid until yabpe_normalize_free, the next
 * yabpe_normalize or yabpe_destroy): *out_dev_text = *out_n_bytes bytes in device memory, *out_dev_part_off = n_parts + 1
 * offsets into them (device memory) -- they can be passed on as the chunk starts of yabpe_pretokenize or the document starts
 * of yabpe_encode.  n_bytes == 0 and empty parts are valid.
 * The rule (csrc/nfc_logic.h): a SEGMENT starts at every code point with canonical combining class 0 and NFC quick-check Yes,
 * and at every part start; a segment is clean (NFC leaves it as it is) iff it holds no code point with quick-check No or
 * Maybe and no adjacent pair with ccc(prev) > ccc(cur) > 0.  A text without such a suspect -- almost every corpus -- costs one
 * pass: *out_dev_text is then `text` itself when that is a device pointer (else the staged copy) and the offsets are
 * unchanged.  Otherwise only the dirty segments are walked (one lane each, forward), everything else is copied; the result
 * is at most 3 n_bytes long.
 * Malformed UTF-8: YABPE_E_UTF8 and *out_bad_pos = UnicodeDecodeError.start of the first bad part, as yabpe_pretokenize
 * reports it (a part cut inside a sequence is malformed on both sides).
 * Cap: a dirty segment of more than 16,384 input code points (a base with thousands of combining marks; the Stream-Safe
 * format of UAX #15 allows 30) makes the call fail with YABPE_E_CAPACITY, *out_bad_pos = the byte position of the segment's
 * start in the INPUT.  Clean segments have no cap. */
#define YABPE_NORM_NFC 1u
int yabpe_normalize(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts,
                    uint32_t form, const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes,
                    int64_t *out_bad_pos);
int yabpe_normalize_free(yabpe_ctx *ctx);
/* What the last yabpe_normalize saw, and the device time of its phases (HIP events around each phase's launches). */
typedef struct yabpe_normalize_stats_t {
    uint64_t n_bytes_in, n_bytes_out, n_parts;
    uint64_t n_suspects;       /* code points that fail the quick check (0: the clean path) */
    uint64_t n_dirty;          /* segments that hold one */
    uint64_t n_dirty_long;     /* ... of them longer than 32 code points after decomposition (one wave each) */
    uint64_t n_copied;         /* bytes the copy pass moved (0 on the clean path) */
    double class_ms;           /* part marks, UTF-8 check, suspects */
    double find_ms;            /* meta bytes, max-scan of the segment starts, the list of dirty segments */
    double segments_ms;        /* lengths of the dirty segments and their scan */
    double write_ms;           /* copy, the segments' bytes, the part offsets */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_normalize_stats_t;
int yabpe_normalize_stats(yabpe_ctx *ctx, yabpe_normalize_stats_t *out);

/* Text with invalid UTF-8 (the step in front of the normaliser) ---------------------------------------
 * errors="replace" / "ignore" on the device: every part [part_off[k], part_off[k+1]) of `text` (read as yabpe_normalize reads
 * them: n_parts ascending starts, the first one 0, the last part ends at n_bytes; part_off == NULL: one part) is replaced by
 * part.decode("utf-8", errors).encode("utf-8") of CPython: every maximal subpart of an ill-formed sequence becomes U+FFFD
 * (EF BF BD, YABPE_UTF8_REPLACE) or is dropped (YABPE_UTF8_IGNORE); any other mode: YABPE_E_INVALID.  Parts are texts of
 * their own: a sequence cut off by a part's end is ill-formed there and never joins the next part (csrc/utf8_logic.h).
 * text may be host or device memory.  Results (owned by the library, valid until yabpe_utf8_repair_free, the next
 * yabpe_utf8_repair or yabpe_destroy): *out_dev_text = *out_n_bytes bytes in device memory (at most 3 x n_bytes, possibly 0),
 * *out_dev_part_off = n_parts + 1 offsets into them (device memory) -- they can be passed on to yabpe_normalize,
 * yabpe_pretokenize or yabpe_encode.  n_bytes == 0 and empty parts are valid.  A text without an ill-formed byte comes back
 * after one pass as it is: *out_dev_text = text when that is device memory (else its staged copy), the offsets the input's. */
#define YABPE_UTF8_REPLACE 1u
#define YABPE_UTF8_IGNORE 2u
int yabpe_utf8_repair(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts,
                      uint32_t mode, const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes);
int yabpe_utf8_repair_free(yabpe_ctx *ctx);
/* What the last yabpe_utf8_repair saw, and the device time of its passes (HIP events around each pass's launches). */
typedef struct yabpe_utf8_stats_t {
    uint64_t n_bytes_in, n_bytes_out, n_parts;
    uint64_t n_subparts;       /* maximal subparts replaced or dropped (0: the valid path) */
    int64_t first_bad_pos;     /* byte position of the first one in the input, -1: none */
    double check_ms;           /* part lookup, charges, tile sums */
    double write_ms;           /* scan of the tile sums, the text, the part offsets */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_utf8_stats_t;
int yabpe_utf8_repair_stats(yabpe_ctx *ctx, yabpe_utf8_stats_t *out);

/* Lower-case text (the step between the repair and the normaliser) -----------------------------------
 * str.lower() on the device: every part [part_off[k], part_off[k+1]) of `text` (read as yabpe_normalize reads them: n_parts
 * ascending starts, the first one 0, the last part ends at n_bytes; part_off == NULL: one part) is replaced by part.lower()
 * of CPython, Unicode version as csrc/unicode_case.inc says (generated by tools/gen_unicode_case.py from the installed
 * interpreter).  Parts are lowered independently: the final-sigma rule -- the one rule of str.lower() that looks at the
 * neighbours -- never looks across a part boundary (csrc/case_logic.h).
 * text may be host or device memory.  Results (owned by the library, valid until yabpe_lowercase_free, the next
 * yabpe_lowercase or yabpe_destroy): *out_dev_text = *out_n_bytes bytes in device memory (at most 1.5 x n_bytes, possibly 0),
 * *out_dev_part_off = n_parts + 1 offsets into them (device memory) -- they can be passed on to yabpe_normalize,
 * yabpe_pretokenize or yabpe_encode.  n_bytes == 0 and empty parts are valid.  One pass counts what changes; then
 *   path 0  nothing does: *out_dev_text = text when that is 16-byte aligned device memory (else its staged copy), the offsets
 *           the input's;
 *   path 1  no code point changes its UTF-8 length and there is no capital sigma: one pass of the same size, the offsets the
 *           input's;
 *   path 2  otherwise: two scans for the final sigmas, a scan of the window sizes, a shifted write.
 * No path has a cap, and none is more than linear in n_bytes whatever the text holds.
 * Malformed UTF-8: YABPE_E_UTF8 and *out_bad_pos = UnicodeDecodeError.start of the first bad part, as yabpe_pretokenize
 * reports it (a part cut inside a sequence is malformed on both sides). */
int yabpe_lowercase(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts,
                    const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes, int64_t *out_bad_pos);
int yabpe_lowercase_free(yabpe_ctx *ctx);
/* What the last yabpe_lowercase saw, and the device time of its phases (HIP events around each phase's launches). */
typedef struct yabpe_lowercase_stats_t {
    uint64_t n_bytes_in, n_bytes_out, n_parts;
    uint64_t n_changed;        /* code points that change (0: path 0) */
    uint64_t n_resized;        /* ... of them whose UTF-8 length changes */
    uint64_t n_sigma;          /* capital sigmas */
    uint64_t n_final_sigma;    /* ... of them that became final sigmas */
    uint64_t path;             /* 0 same pointer, 1 same size, 2 general */
    uint64_t n_copied;         /* bytes a write pass stored (0 on path 0) */
    double check_ms;           /* part marks, UTF-8 check, counters, window sizes */
    double scan_ms;            /* path 2: the two final-sigma scans, the scan of the window sizes */
    double write_ms;           /* path 1: the same-size pass; path 2: the shifted write and the part offsets */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_lowercase_stats_t;
int yabpe_lowercase_stats(yabpe_ctx *ctx, yabpe_lowercase_stats_t *out);

/* Word pool (corpora larger than device memory) -----------------------------------------------------
 * The word-frequency pooling of trainer.py:221-225 (word_freq[word_tuple] += 1 over all sequences) as a structure that
 * persists across calls: the context keeps the multiset of distinct byte strings seen so far with u64 counts, on the device.
 * Text goes through in bounded batches (yabpe_pretokenize -> yabpe_pool_add -> yabpe_pretokenize_free), and the merge loop is
 * loaded from the pool at the end.  The pool needs no vocab and is independent of the loaded corpus: yabpe_load_words leaves
 * it alone, and the pool calls leave the corpus alone.
 *   yabpe_pool_add   adds every word's count to the pool.  The arguments are read as yabpe_load_words reads them: pointers
 *       may be host or device memory (yabpe_pretokenize's results go in as they are), word_off may point into the middle of
 *       a larger array, word_freq == NULL means every word counts once.  Zero-length words are dropped (trainer.py:170, 211)
 *       and counted in the stats.  n_words == 0 is a valid no-op.  YABPE_E_INVALID: word_off is NULL, or bytes is NULL while
 *       the words have bytes.  YABPE_E_CAPACITY: 2^32 - 2 words or more in one call; the pool would pass 2^32 - 2 unique
 *       words (yabpe_load_words's own limit); a word of 2^32 bytes or more.  A failed call leaves the pool as it was.
 *   yabpe_pool_get   the pool as the three arrays yabpe_load_words and yabpe_load_words_resumed take: *out_n_unique + 1
 *       offsets from 0, *out_n_bytes bytes, *out_n_unique u64 counts -- device memory owned by the library, valid until the
 *       next yabpe_pool_add, yabpe_pool_clear or yabpe_destroy.  The order of the words is unspecified (within a call it
 *       follows which occurrence won a race); the trained model does not depend on it.  Before any add: *out_n_unique = 0
 *       (and one offset, 0).  The load COPIES what it needs (the tiles and the long-word buffer are built from the arrays,
 *       and every temporary of the load is gone when it returns), so the pool may be cleared right after yabpe_load_words /
 *       yabpe_load_words_resumed returns.  A count above 2^32 - 1 is the load's YABPE_E_CAPACITY, as for any word_freq.
 *   yabpe_pool_clear frees the pool; the next add starts an empty one (and reads the options again).
 * Options (read when a pool starts): "pool_init_slots" (65,536) and "pool_init_bytes" (1 MiB): the starting capacities of
 * the slot array (rounded up to a power of two, at least 2) and of the byte arena; "pool_hash_bits" (64): only the low N
 * bits of a word's hash are used for placement and for the hash pre-check (0: every word on one probe chain; for tests). */
int yabpe_pool_add(yabpe_ctx *ctx, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words);
int yabpe_pool_get(yabpe_ctx *ctx, const uint8_t **out_dev_bytes, const uint64_t **out_dev_off, const uint64_t **out_dev_freq,
                   uint64_t *out_n_unique, uint64_t *out_n_bytes);
int yabpe_pool_clear(yabpe_ctx *ctx);
/* The pool since it started, and the device time of the last add that had words (HIP events around each phase's launches). */
typedef struct yabpe_pool_stats_t {
    uint64_t n_calls;          /* yabpe_pool_add calls that succeeded, empty ones included */
    uint64_t n_words_added;    /* words those calls passed (entries of word_off, zero-length ones included) */
    uint64_t n_empty_dropped;  /* occurrences of zero-length words dropped (with word_freq: their frequencies) */
    uint64_t n_unique;         /* words in the pool */
    uint64_t n_bytes;          /* their bytes */
    uint64_t slot_capacity;    /* slots (>= 2 n_unique); the per-word arrays hold slot_capacity / 2 words */
    uint64_t arena_capacity;   /* bytes the arena holds */
    uint64_t slot_growths;     /* times the slots (and the per-word arrays with them) were reallocated and refilled */
    uint64_t arena_growths;    /* times the arena was reallocated */
    double pool_ms;            /* the call-local pooling of equal words */
    double probe_ms;           /* list of the call's unique words, their lookup, scans of the new ones */
    double append_ms;          /* growth (copies, re-insertion) and the append */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_pool_stats_t;
int yabpe_pool_stats(yabpe_ctx *ctx, yabpe_pool_stats_t *out);

/* Encoder (BBPETokenizer.encode on the device, yet_another_bpe/tokenizer.py) ----------------------------------------
 * A trained model: the vocab (n_vocab byte strings, vocab_off: n_vocab + 1 offsets, vocab_ids: their ids), the merges in
 * order (merge_off: 2 n_merges + 1 offsets, left and right operand of merge i = entries 2i and 2i + 1) and the specials in
 * the tokenizer's order (longest first, stable).  unk_id = vocab.get(b"[UNK]", 0).  The library interns every byte string
 * that can be a token (single bytes, both operands and the concatenation of every merge) and keeps the pair table, the
 * id map and the specials on the device.  Rejects an empty special (YABPE_E_INVALID) and more than 254 specials
 * (YABPE_E_CAPACITY).  Ids are u32. */
int yabpe_encode_set_model(yabpe_ctx *ctx, const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids,
                           uint32_t n_vocab, const uint8_t *merge_bytes, const uint64_t *merge_off, uint32_t n_merges,
                           const uint8_t *special_bytes, const uint32_t *special_off, uint32_t n_special, uint32_t unk_id);
/* Encodes n_docs documents: document d = text[doc_off[d], doc_off[d + 1]) (the last one ends at n_bytes; doc_off[0] = 0,
 * ascending; text host or device memory), each exactly as a separate BBPETokenizer.encode call would.  Results (device
 * memory owned by the library, released by yabpe_encode_free, the next yabpe_encode or yabpe_destroy): *out_dev_ids =
 * *out_n_ids u32 ids, *out_dev_doc_off = n_docs + 1 offsets into them.  Malformed UTF-8: YABPE_E_UTF8 and *out_bad_pos =
 * UnicodeDecodeError.start of the whole text.  More than 2^32 - 1 pre-tokens in one call: YABPE_E_CAPACITY.
 * Option "digit_group" (see yabpe_pretokenize): the pre-tokens of the text between the specials are those of the grouped
 * pattern, in yabpe_encode, yabpe_encode_spans and yabpe_encode_dropout alike -- BBPETokenizer(digit_group=G).  The specials
 * are split out first and every piece between them is a text of its own, so here a special may begin with a digit.
 * Option "split_pattern" (see yabpe_pretokenize) likewise: 1 gives the pre-tokens of the cl100k pattern in all three calls --
 * BBPETokenizer(pretokenizer="cl100k") -- and here a special may begin with whitespace too; 3 gives those of the o200k_base
 * pattern -- BBPETokenizer(pretokenizer="o200k_base") -- and here the specials are unrestricted. */
int yabpe_encode(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs,
                 uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint64_t *out_n_ids, int64_t *out_bad_pos);
/* yabpe_encode that also says which piece of its document every id was made from.  Arguments, errors and ownership are
 * yabpe_encode's; flags: 0 or YABPE_SPANS_CHARS (anything else: YABPE_E_INVALID).  *out_dev_spans = 2 * *out_n_ids u64,
 * interleaved (start, end) per id, relative to the start of the id's document (device memory owned by the library, released
 * by yabpe_encode_free, the next yabpe_encode or yabpe_encode_spans, or yabpe_destroy).  Bytes: the bytes the token was
 * merged from -- also for a token the vocab lacks (the unk id keeps its span); a special with an id spans its occurrence,
 * one without an id emits nothing and leaves a gap; all other spans of a document tile it in ascending order.
 * YABPE_SPANS_CHARS: code-point indices instead, the smallest run of whole characters that covers the token's bytes (with
 * lead(p) = the non-continuation bytes below p: start = lead(start_byte + 1) - 1, end = lead(end_byte)). */
#define YABPE_SPANS_CHARS 0x1u   /* code points instead of bytes */
int yabpe_encode_spans(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs,
                       uint32_t flags, uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint64_t **out_dev_spans,
                       uint64_t *out_n_ids, int64_t *out_bad_pos);
/* yabpe_encode with BPE-dropout (BBPETokenizer.encode_dropout; Provilkov et al., 2020): at every merge step of every
 * pre-token each candidate pair is skipped with probability p = threshold / 2^32, reproducibly from (seed, document index,
 * position): with rnd(seed, stream, i) of yet_another_bpe/synth.py, Kd = rnd(seed, 0x64, d) for document d, Kw =
 * rnd(Kd, 0x77, s) for the pre-token at byte s of its document, and the candidate whose left part starts at byte q of the
 * word is skipped at step t (merges performed so far) iff rnd(Kw, t, q) >> 32 < threshold; the surviving candidate of lowest
 * rank merges, leftmost on ties; no survivor ends the word.  threshold = min(2^32, int(p * 2^32)): 0 gives yabpe_encode's
 * ids, 2^32 one id per byte; above 2^32: YABPE_E_INVALID.  Specials draw nothing.  Arguments, errors, ownership and release
 * are yabpe_encode's, and the results serve wherever its results do (yabpe_decode, yabpe_layout_pad, yabpe_layout_pack).
 * Every occurrence is merged on its own: yabpe_encode_stats reports n_unique = 0 and pool_ms = 0, n_unique_long counts the
 * occurrences longer than 64 bytes, and yabpe_encode_checksum has nothing to report after this call.
 * Option "dropout_pack" (default 1): 0 gives every word of up to 64 bytes a wave of its own (for measurements). */
int yabpe_encode_dropout(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs,
                         uint64_t threshold, uint64_t seed, uint32_t **out_dev_ids, uint64_t **out_dev_doc_off,
                         uint64_t *out_n_ids, int64_t *out_bad_pos);
/* yabpe_encode that also says which piece of its document every id was made from (BBPETokenizer.encode_with_words).  The
 * pieces of a document, in order: every occurrence of a special token, with an id or without, and every match of the split
 * pattern in the text between them.  *out_dev_words = *out_n_ids u32 (device memory owned by the library, released as the
 * ids are): the low 31 bits hold the 0-based index of the id's piece among the pieces of its document, bit 31
 * (YABPE_WORD_SPECIAL) is set when that piece is a special occurrence.  The indices of a document never decrease; a special
 * without an id takes an index and emits nothing, which leaves a gap.  Arguments, errors, ownership and release are
 * yabpe_encode's, the ids and doc_off are bit-identical to its results on the same input, and the options act alike.  A
 * document of 2^31 pieces or more: YABPE_E_CAPACITY. */
#define YABPE_WORD_SPECIAL 0x80000000u   /* words[k]: the piece is a special occurrence */
int yabpe_encode_words(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs,
                       uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint32_t **out_dev_words, uint64_t *out_n_ids,
                       int64_t *out_bad_pos);
int yabpe_encode_free(yabpe_ctx *ctx);
/* What the last yabpe_encode /yabpe_encode_spans / yabpe_encode_dropout saw (the span work counts into words_ms and emit_ms), and the device time of its phases (HIP events around each phase's launches). */
typedef struct yabpe_encode_stats_t {
    uint64_t n_bytes, n_docs;
    uint64_t n_pretokens;      /* pre-tokens, specials included */
    uint64_t n_unique;         /* unique pre-tokens (pooled words) */
    uint64_t n_unique_long;    /* ... of them longer than 64 bytes (the sequential path) */
    uint64_t n_specials;       /* special-token occurrences taken */
    uint64_t n_ids;
    double split_ms;           /* special split + UTF-8 check + pre-token starts */
    double pretok_ms;          /* starts -> pre-token offsets */
    double pool_ms;            /* pre-tokens -> unique words */
    double words_ms;           /* merges of every unique word */
    double emit_ms;            /* ids and document offsets */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_encode_stats_t;
int yabpe_encode_stats(yabpe_ctx *ctx, yabpe_encode_stats_t *out);
/* Debug: yabpe_stream_checksum's fold (FNV over each word's token bytes with the 0x1ff boundary, mixed, summed) over the
 * last yabpe_encode's pre-tokens, specials excluded, that end as at least 2 tokens (the words a flat training stream still
 * holds), plus the number of those pre-tokens and of their tokens. */
int yabpe_encode_checksum(yabpe_ctx *ctx, uint64_t *out_sum, uint64_t *out_words, uint64_t *out_tokens);

/* Decoder (BBPETokenizer.decode on the device, yet_another_bpe/tokenizer.py) ----------------------------------------
 * The vocab as yabpe_encode_set_model takes it (n_vocab byte strings, vocab_off: n_vocab + 1 offsets, vocab_ids: their ids).
 * The library keeps a dense table id -> bytes on the device; when two strings share an id the last one wins (decode's
 * {i: t for t, i in vocab.items()}).  An id above 2^24 - 1 or a vocab of 2^32 - 1 bytes or more: YABPE_E_CAPACITY.
 * Independent of yabpe_encode_set_model. */
int yabpe_decode_set_model(yabpe_ctx *ctx, const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids,
                           uint32_t n_vocab);
/* Decodes n_docs documents: document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids; doc_off[0] = 0,
 * ascending; doc_off == NULL with n_docs <= 1: one document), each exactly as a separate BBPETokenizer.decode call would,
 * as UTF-8: ids the vocab does not name are skipped, and every maximal subpart of an ill-formed sequence becomes U+FFFD
 * (errors="replace"; a sequence cut off at a document's end is replaced there).  ids and doc_off may be host or device
 * memory (yabpe_encode's results can be passed as they are).  Results (device memory owned by the library, released by
 * yabpe_decode_free, the next yabpe_decode or yabpe_destroy): *out_dev_text = *out_n_bytes bytes, *out_dev_text_off =
 * n_docs + 1 offsets into them.  No model: YABPE_E_INVALID. */
int yabpe_decode(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                 uint8_t **out_dev_text, uint64_t **out_dev_text_off, uint64_t *out_n_bytes);
int yabpe_decode_free(yabpe_ctx *ctx);
/* What the last yabpe_decode saw, and the device time of its phases (HIP events around each phase's launches). */
typedef struct yabpe_decode_stats_t {
    uint64_t n_ids, n_docs;
    uint64_t n_unknown;        /* ids skipped: not in the table */
    uint64_t n_gathered;       /* bytes of the known ids' tokens */
    uint64_t n_bytes;          /* bytes out */
    uint64_t n_replacements;   /* U+FFFD written */
    uint64_t n_docs_repaired;  /* documents with at least one U+FFFD */
    double lengths_ms;         /* per-block byte counts + their scan */
    double gather_ms;          /* token bytes -> text, document offsets */
    double check_ms;           /* UTF-8 roles and the U+FFFD count */
    double repair_ms;          /* 0 when the text was valid: scan + rewrite with U+FFFD */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_decode_stats_t;
int yabpe_decode_stats(yabpe_ctx *ctx, yabpe_decode_stats_t *out);

/* Fixed-shape batches (BBPETokenizer.encode_batch_padded / encode_batch_packed on the device) -----------------------
 * ids and doc_off are taken as yabpe_decode takes them: document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at
 * n_ids; doc_off[0] = 0, ascending; doc_off == NULL with n_docs <= 1: one document), host or device memory; yabpe_encode's
 * results can be passed as they are and are left alone.  No model is needed.  With seq(d) = [bos_id] + the document's ids +
 * [eos_id] (YABPE_LAYOUT_BOS / _EOS say which of the two are given; n_added = how many):
 *   yabpe_layout_pad   one row of row_len slots per document.  A seq(d) longer than row_len loses ids from the end of its
 *       content (YABPE_LAYOUT_TRUNC_LEFT: from the start); BOS and EOS always survive.  *out_dev_len[d] = the length after the
 *       cut.  The kept sequence sits at the left end of its row (YABPE_LAYOUT_PAD_LEFT: at the right end), pad_id elsewhere.
 *       row_len == 0: the longest seq(d), found on the device; *out_row_len = the row length used.
 *       Results: *out_dev_rows = n_docs * *out_row_len u32, *out_dev_len = n_docs u32.
 *   yabpe_layout_pack  all seq(d) end to end in document order, cut into rows of row_len: *out_n_rows = ceil(stream /
 *       row_len) rows, or floor with YABPE_LAYOUT_DROP_LAST (the last partial row is dropped).  Per slot: the id, the index
 *       of the document it came from, and its index inside seq(d) (BOS is 0).  Slots of the last row past the stream:
 *       pad_id, document 0xFFFFFFFF, position 0.  Results: three arrays of *out_n_rows * row_len u32.
 * Results are device memory owned by the library, in buffers of their own (a later yabpe_encode leaves them valid), released
 * by yabpe_layout_free, the next layout call or yabpe_destroy.
 * YABPE_E_INVALID: flags outside YABPE_LAYOUT_*, or one that does not belong to the call (TRUNC_LEFT / PAD_LEFT: pad only;
 * DROP_LAST: pack only); 0 < row_len < n_added for pad; row_len == 0 for pack; doc_off that does not ascend from 0 inside the
 * ids.  YABPE_E_CAPACITY: more than 2^36 output slots in one call; a seq(d) of more than 2^32 - 1 entries (pack: positions
 * are u32; pad with row_len == 0: so is the row length). */
#define YABPE_LAYOUT_BOS        0x01u
#define YABPE_LAYOUT_EOS        0x02u
#define YABPE_LAYOUT_TRUNC_LEFT 0x04u
#define YABPE_LAYOUT_PAD_LEFT   0x08u
#define YABPE_LAYOUT_DROP_LAST  0x10u
typedef struct yabpe_layout_t {
    uint32_t row_len;  /* pad: max_length (0: the longest sequence); pack: seq_len */
    uint32_t pad_id, bos_id, eos_id;  /* bos_id / eos_id are read only with their flag */
    uint32_t flags;    /* YABPE_LAYOUT_* */
} yabpe_layout_t;
int yabpe_layout_pad(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                     const yabpe_layout_t *layout, uint32_t **out_dev_rows, uint32_t **out_dev_len, uint32_t *out_row_len);
int yabpe_layout_pack(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                      const yabpe_layout_t *layout, uint32_t **out_dev_ids, uint32_t **out_dev_doc, uint32_t **out_dev_pos,
                      uint64_t *out_n_rows);
/* Overlapping windows (BBPETokenizer.encode_batch_windows on the device): a document longer than a row becomes several rows.
 * ids, doc_off and layout as the two calls above take them; layout->row_len = max_length, flags: YABPE_LAYOUT_BOS / _EOS /
 * _PAD_LEFT.  With C = row_len - n_added content slots a row and step = C - stride: row k = 0, 1, ... of document d holds
 * [bos_id] + ids[k * step : k * step + C] + [eos_id], padded with pad_id at its right end (YABPE_LAYOUT_PAD_LEFT: at its left
 * end); the last row of a document is the first one with k * step + C >= n.  Every document, an empty one included, has at
 * least one row: 1 for n <= C, else 1 + ceil((n - C) / step); every row but a document's last is full, and consecutive rows of
 * a document share exactly stride ids.  Rows are in document order, in window order within a document.
 * Results (device memory owned by the library, buffers of their own, released as the other layout results are): rows = n_rows
 * * row_len u32; per row its document (row_doc), k * step (row_start: the index of its first content id in the document) and
 * its length before padding, BOS / EOS included (row_len).  spans: NULL, or 2 * n_ids u64 as yabpe_encode_spans returns them
 * (host or device memory); then out->spans = 2 * n_rows * row_len u64, the (start, end) of every slot's id, (0, 0) in BOS, EOS
 * and pad slots; without spans out->spans = NULL.
 * YABPE_E_INVALID: row_len <= n_added; stride >= row_len - n_added; YABPE_LAYOUT_TRUNC_LEFT, _DROP_LAST or an unknown flag; a
 * bad doc_off.  YABPE_E_CAPACITY: more than 2^36 output slots; a document of more than 2^32 - 1 ids.  Every error is found
 * before a result buffer is allocated.  yabpe_layout_stats: n_truncated_docs = the documents of more than one row,
 * n_ids_dropped = 0, lengths_ms = row counts + their scan + the row records. */
typedef struct yabpe_windows_t {
    uint32_t *rows;       /* n_rows * row_len */
    uint32_t *row_doc;    /* n_rows */
    uint32_t *row_start;  /* n_rows */
    uint32_t *row_len;    /* n_rows */
    uint64_t *spans;      /* 2 * n_rows * row_len, or NULL */
    uint64_t n_rows;
} yabpe_windows_t;
int yabpe_layout_windows(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                         const uint64_t *spans, const yabpe_layout_t *layout, uint32_t stride, yabpe_windows_t *out);
/* Text pairs (BBPETokenizer.encode_batch_pairs on the device): documents 2p and 2p + 1 are the two sides A, B of pair p and
 * share rows.  ids, doc_off and spans as yabpe_layout_windows takes them (host or device memory; the encoder's results pass
 * straight in and are left alone); no model is needed.  layout->row_len = max_length, flags: YABPE_LAYOUT_BOS / _EOS /
 * _PAD_LEFT.  n_added = BOS + EOS + pairs->n_sep (0, 1 or 2 copies of sep_id between the sides), C = row_len - n_added.
 * A row holds [bos_id] + A[:ka] + [sep_id] * n_sep + B[s : s + kb] + [eos_id], padded with pad_id at its right end
 * (YABPE_LAYOUT_PAD_LEFT: at its left end).  The truncation modes give row p = pair p with s = 0; ids leave from the END of a
 * side and every row fits:
 *   YABPE_PAIRS_LONGEST_FIRST  while ka + kb > C the longer side loses its last id, the second when both are equally long;
 *   YABPE_PAIRS_ONLY_FIRST     the first gives up the excess la + lb - C, down to zero ids; a second still longer than C is
 *                              cut to C;    YABPE_PAIRS_ONLY_SECOND: the mirror image.
 *   YABPE_PAIRS_WINDOWS        (0 <= stride <= C - 1) ka = min(la, C - stride - 1) in every row of the pair; the second side
 *       is windowed as yabpe_layout_windows does with Cb = C - ka content slots and step = Cb - stride: row k has s = k * step
 *       and kb = min(Cb, lb - s), the last row is the first with s + Cb >= lb; at least one row a pair.  Rows are in pair
 *       order, in window order within a pair.
 * Results (device memory owned by the library, buffers of their own: a later yabpe_encode leaves them valid; released by
 * yabpe_layout_free, the next layout call or yabpe_destroy): rows and types (0: BOS, the first side, separators, padding; 1:
 * the second side and EOS) per slot; per row its pair, s, ka and kb (the length before padding is ka + kb + n_added); with
 * spans (2 * n_ids u64 as yabpe_encode_spans returns them) out->spans = the (start, end) of every slot's id in its own
 * document, (0, 0) in BOS, separator, EOS and pad slots; without, out->spans = NULL.  n_docs = 0: no rows.
 * YABPE_E_INVALID: an odd n_docs; row_len <= n_added; n_sep > 2; an unknown mode; stride != 0 outside windows mode; stride >=
 * C in windows mode; YABPE_LAYOUT_TRUNC_LEFT, _DROP_LAST or an unknown flag; a bad doc_off.  YABPE_E_CAPACITY: more than 2^36
 * output slots; a document of more than 2^32 - 1 ids.  Every error is found before a result buffer is allocated.
 * yabpe_layout_stats: n_docs counts documents (two a pair); n_truncated_docs = the pairs that lost an id or took more than one
 * row; n_ids_dropped = the ids cut away in the truncation modes, 0 in windows mode; lengths_ms = the counters, in windows mode
 * the row counts and their scan, and the row records. */
#define YABPE_PAIRS_LONGEST_FIRST 0u
#define YABPE_PAIRS_ONLY_FIRST    1u
#define YABPE_PAIRS_ONLY_SECOND   2u
#define YABPE_PAIRS_WINDOWS       3u
typedef struct yabpe_pairs_t { uint32_t sep_id, n_sep, mode, stride; } yabpe_pairs_t;
typedef struct yabpe_pair_rows_t {
    uint32_t *rows;        /* n_rows * row_len */
    uint8_t  *types;       /* n_rows * row_len */
    uint32_t *row_pair, *row_start, *first_len, *second_len;   /* n_rows each */
    uint64_t *spans;       /* 2 * n_rows * row_len, or NULL */
    uint64_t n_rows;
} yabpe_pair_rows_t;
int yabpe_layout_pairs(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                       const uint64_t *spans, const yabpe_layout_t *layout, const yabpe_pairs_t *pairs, yabpe_pair_rows_t *out);
/* Whole documents (BBPETokenizer.encode_batch_fit on the device): rows of row_len slots that hold whole sequences, packed by
 * best-fit decreasing; no sequence is cut across two rows.  ids, doc_off and layout as the calls above take them (host or device
 * memory; the encoder's results pass straight in and are left alone); no model is needed.  flags: YABPE_LAYOUT_BOS / _EOS.
 * With C = row_len: a seq(d) longer than C loses content ids from its end as in yabpe_layout_pad (BOS and EOS survive), n_d =
 * min(len(seq(d)), C); a document with n_d == 0 takes no slot and is in no row.
 * Plan: H[k] = the documents with n_d == k.  The state maps a shape (the sequence lengths of a row in placement order, non-
 * increasing; room(s) = C - sum(s)) to the number of rows that have it.  For k = C down to 1 with n = H[k] sequences left: among
 * the shapes with a row left and room >= k the one with the smallest room, of several the lexicographically greatest; with t =
 * room / k, min(rows, n / t) rows of it take t sequences each and, if rows of it and sequences remain, one more row takes the
 * rest; with no such shape n / t rows of t = C / k sequences open and one row of the n % t left.  Rows: the shapes in descending
 * tuple order, the rows of a shape consecutive; a row holds its sequences end to end from column 0, then pad_id.  For every k the
 * documents with n_d == k, in ascending d, take the places of length k in row order, within a row left to right.  The rows use
 * no more room than best-fit decreasing one document at a time, and the result depends on the documents alone.
 * Results (device memory owned by the library, buffers of their own, released as the other layout results are): per slot the id,
 * the document it came from and its index inside seq(d) as yabpe_layout_pack gives them (pad slots: pad_id, 0xFFFFFFFF, 0);
 * used[r] = the filled slots of row r.  n_docs = 0, or only empty sequences: no rows.
 * YABPE_E_INVALID: row_len == 0, row_len < n_added or row_len > 2^24 - 1 (the sort keys have three 8-bit digits); any flag but
 * YABPE_LAYOUT_BOS / _EOS; a bad doc_off.  YABPE_E_CAPACITY: more than 2^36 output slots.  Every error is found before a result
 * buffer is allocated.  yabpe_layout_stats: n_truncated_docs, n_ids_dropped and n_pad_slots as for yabpe_layout_pad; lengths_ms =
 * lengths + histogram + sort, write_ms = the output pass, total_ms includes the plan, which runs on the host. */
typedef struct yabpe_fit_rows_t {
    uint32_t *ids, *doc, *pos;   /* n_rows * row_len each */
    uint32_t *used;              /* n_rows */
    uint64_t n_rows;
} yabpe_fit_rows_t;
int yabpe_layout_fit(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                     const yabpe_layout_t *layout, yabpe_fit_rows_t *out);
int yabpe_layout_free(yabpe_ctx *ctx);
/* What the last yabpe_layout_pad / yabpe_layout_pack / yabpe_layout_windows / yabpe_layout_pairs / yabpe_layout_fit saw, and the device time of
 * its phases (HIP events around each phase's launches). */
typedef struct yabpe_layout_stats_t {
    uint64_t n_ids, n_docs;
    uint64_t n_rows, row_len;
    uint64_t n_truncated_docs; /* pad: documents whose seq was cut */
    uint64_t n_ids_dropped;    /* pad: ids cut away; pack: stream entries of the row YABPE_LAYOUT_DROP_LAST dropped */
    uint64_t n_pad_slots;      /* slots that hold pad_id */
    double lengths_ms;         /* kept lengths and the call's counters (pad) / stream offsets (pack) */
    double write_ms;           /* the output pass */
    double total_ms;           /* first to last event, host gaps in between included */
} yabpe_layout_stats_t;
int yabpe_layout_stats(yabpe_ctx *ctx, yabpe_layout_stats_t *out);

/* Masked-language-model batches (BBPETokenizer.mask_tokens on the device, yet_another_bpe/tokenizer.py) --------------
 * From ragged ids, document d = ids[doc_off[d], doc_off[d + 1]) (the last one ends at n_ids; doc_off: n_docs starts, the first
 * one 0, ascending; NULL with n_docs <= 1: one document), to the `input_ids` and `labels` of one dynamic-masking draw,
 * reproducibly from (seed, document index, position).  With rnd(seed, stream, i) of yet_another_bpe/synth.py: Kd =
 * rnd(seed, 0x6d, first_doc + d) for document d.  For token j of the document (0-based, counted before any cut of a layout
 * call) the unit is u = j, with YABPE_MASK_WHOLE_WORD u = words[k] & 0x7FFFFFFF, the piece the id was made from.  A token
 * whose words entry has YABPE_WORD_SPECIAL set is never selected and draws nothing.  Otherwise r = rnd(Kd, 0x73, u), and the
 * token is selected iff (r >> 32) < select_threshold.  For a selected token the label is the original id, and x = r &
 * 0xFFFFFFFF decides the input: x < mask_threshold: mask_id; mask_threshold <= x < mask_threshold + random_threshold:
 * rnd(Kd, 0x72, j) % n_random (drawn per token in whole-word mode too); otherwise the id stays.  For every other token the id
 * stays and the label is `ignore`.  A threshold is T(x) = min(2^32, int(x * 2^32)) of a probability x.  Every draw is a function
 * of (seed, first_doc + d, u or j) alone, so all tokens of a word are selected together and replaced in the same way.
 * ids, doc_off and words may be host or device memory, as in the layout calls; yabpe_encode_words' results go straight in and
 * are left alone.  words: what yabpe_encode_words returns, flag bit included, or NULL: nothing is protected (invalid with
 * YABPE_MASK_WHOLE_WORD).  Results (device memory owned by the library, in buffers of their own: a later encode or layout call
 * leaves them valid; released by yabpe_mask_free, the next yabpe_mask or yabpe_destroy): *out_dev_ids and *out_dev_labels,
 * n_ids u32 each.  YABPE_E_INVALID: a threshold above 2^32, mask_threshold + random_threshold above 2^32, n_random == 0 with
 * random_threshold > 0, an unknown flag, YABPE_MASK_WHOLE_WORD without words, a doc_off that does not ascend from 0 inside the
 * ids.  YABPE_E_CAPACITY: more than 2^36 ids in one call.  Every error is found before a buffer is allocated. */
#define YABPE_MASK_WHOLE_WORD 0x1u   /* the unit of selection is the piece (words), not the token */
typedef struct yabpe_mask_t {
    uint64_t seed, first_doc;
    uint64_t select_threshold;                 /* Ts, <= 2^32 */
    uint64_t mask_threshold, random_threshold; /* Tm, Tr; Tm + Tr <= 2^32 */
    uint32_t mask_id, n_random;                /* n_random >= 1 when Tr > 0 */
    uint32_t ignore;                           /* the label of an unselected slot (0xFFFFFF9C is -100 as i32) */
    uint32_t flags;                            /* YABPE_MASK_WHOLE_WORD */
} yabpe_mask_t;
int yabpe_mask(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
               const uint32_t *words, const yabpe_mask_t *mask, uint32_t **out_dev_ids, uint32_t **out_dev_labels);
int yabpe_mask_free(yabpe_ctx *ctx);
/* What the last yabpe_mask saw and drew, and its device time. */
typedef struct yabpe_mask_stats_t {
    uint64_t n_ids, n_docs;
    uint64_t n_protected;      /* ids of special occurrences (never selected) */
    uint64_t n_selected;       /* = n_masked + n_random + n_kept */
    uint64_t n_masked;         /* inputs that became mask_id */
    uint64_t n_random;         /* inputs that became a random id */
    uint64_t n_kept;           /* selected, input unchanged */
    double mask_ms;            /* the kernel */
    double total_ms;           /* first to last event (counter reset and read-back included) */
} yabpe_mask_stats_t;
int yabpe_mask_stats(yabpe_ctx *ctx, yabpe_mask_stats_t *out);

/* Span-corruption batches (BBPETokenizer.corrupt_spans on the device, yet_another_bpe/tokenizer.py) -------------------
 * The encoder-decoder denoising objective (T5 / UL2 / SpanBERT style): contiguous spans leave the input, one sentinel
 * stands for each, and the target lists the sentinels with the ids they stand for.  ids, doc_off, n_docs and words as
 * yabpe_mask takes them, host or device memory; yabpe_encode_words' results go straight in and are left alone.
 * The rule, with rnd(seed, stream, i) of yet_another_bpe/synth.py: Kd = rnd(seed, 0x63, first_doc + d) for document d.  For
 * token j of the document (0-based, counted before any cut) the unit is u = j, with YABPE_SPAN_WHOLE_WORD u = words[k] &
 * 0x7FFFFFFF.  Per unit r = rnd(Kd, 0x6f, u): the unit opens a span iff (r >> 32) < open_threshold, and the span covers
 * len(u) = 1 + #{k < max_len - 1 : (r & 0xFFFFFFFF) < len_threshold[k]} units from u on.  Unit v is noise iff some u in
 * [max(0, v - max_len + 1), v] opens with u + len(u) > v; overlapping and adjacent spans merge.  A token is noise iff its unit
 * is noise and its words entry has no YABPE_WORD_SPECIAL: specials are never removed, and they split runs.  No draw reads
 * protection, the cut or the batch.  max_doc_ids (0: none): ids with j >= max_doc_ids appear in neither output.
 * A run is a maximal stretch of consecutive kept noise ids of one document; the runs of a document are numbered k = 0, 1, ...
 * With K = n_sentinels - (1 with YABPE_SPAN_FINAL_SENTINEL), the runs k >= K are not corrupted: their ids stay in the input and
 * nothing of them goes to the target.  Per document, inputs: the kept ids in order, every run k < K replaced by
 * sentinels[k]; targets: for every run k < K, sentinels[k] and then the run's ids; with YABPE_SPAN_FINAL_SENTINEL, then
 * sentinels[min(n_runs, K)] if the document keeps at least one id.  An empty document gives two empty sequences.
 * Results (device memory owned by the library, in buffers of their own: a later encode, mask or layout call leaves them
 * valid; released by yabpe_span_free, the next yabpe_span_corrupt or yabpe_destroy): *out_dev_in, u32[*out_n_in], with
 * *out_dev_in_off, u64[n_docs + 1], and the same for the targets -- what the layout calls take as ids and doc_off.
 * YABPE_E_INVALID: open_threshold or a len_threshold above 2^32, len_threshold increasing, max_len outside 1 ..
 * YABPE_SPAN_MAX_LEN, n_sentinels == 0 (== 1 with the final sentinel) or sentinels NULL, an unknown flag,
 * YABPE_SPAN_WHOLE_WORD without words, a doc_off that does not ascend from 0 inside the ids.  YABPE_E_CAPACITY: more than
 * 2^36 ids in one call.  Every error is found before a buffer is allocated. */
#define YABPE_SPAN_MAX_LEN 32
#define YABPE_SPAN_WHOLE_WORD 0x1u       /* the unit of the draws is the piece (words), not the token */
#define YABPE_SPAN_FINAL_SENTINEL 0x2u   /* the targets of a document end with one more sentinel */
typedef struct yabpe_span_t {
    uint64_t seed, first_doc;
    uint64_t open_threshold;                          /* To, <= 2^32 */
    uint64_t len_threshold[YABPE_SPAN_MAX_LEN - 1];   /* C[0 .. max_len - 2], <= 2^32, non-increasing; the rest is not read */
    uint32_t max_len;                                 /* Lmax, 1 .. YABPE_SPAN_MAX_LEN */
    uint32_t n_sentinels;
    const uint32_t *sentinels;                        /* n_sentinels ids, host memory */
    uint64_t max_doc_ids;                             /* 0: no cut */
    uint32_t flags;                                   /* YABPE_SPAN_* */
} yabpe_span_t;
int yabpe_span_corrupt(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs,
                       const uint32_t *words, const yabpe_span_t *span, uint32_t **out_dev_in, uint64_t **out_dev_in_off,
                       uint64_t *out_n_in, uint32_t **out_dev_tgt, uint64_t **out_dev_tgt_off, uint64_t *out_n_tgt);
int yabpe_span_free(yabpe_ctx *ctx);
/* What the last yabpe_span_corrupt saw and drew, and its device time. */
typedef struct yabpe_span_stats_t {
    uint64_t n_ids, n_docs;
    uint64_t n_protected;      /* ids of special occurrences (never noise) */
    uint64_t n_noise;          /* kept ids that are noise, those of runs past the cap included */
    uint64_t n_runs;           /* runs, those past the cap included */
    uint64_t n_runs_over;      /* runs past the sentinel cap (left in the inputs) */
    uint64_t n_cut;            /* ids at or past max_doc_ids */
    uint64_t n_in, n_tgt;      /* ids of the inputs / the targets, sentinels included */
    double flags_ms;           /* the draws: a byte per id */
    double index_ms;           /* run numbers, the sentinel cap, slots per id */
    double place_ms;           /* the two position scans and the document offsets */
    double write_ms;           /* the output pass */
    double kernel_ms;          /* the four together */
    double total_ms;           /* first to last event (counter reset, read-backs and allocation included) */
} yabpe_span_stats_t;
int yabpe_span_stats(yabpe_ctx *ctx, yabpe_span_stats_t *out);

/* Fill-in-the-middle batches (BBPETokenizer.fim_tokens / fim_cuts on the device, yet_another_bpe/tokenizer.py) ---------
 * The objective of decoder-only code models (Bavarian et al., 2022): a document is cut at two random places into prefix,
 * middle and suffix and written as "pre P suf S mid M [eot]" (PSM) or "pre suf S mid P M [eot]" (SPM, the variant with
 * prefix and middle adjacent).  The rule, with rnd(seed, stream, i) of yet_another_bpe/synth.py: Kd = rnd(seed, 0x66,
 * first_doc + d) for document d; r = rnd(Kd, 0x61, 0): the document is transformed iff (r >> 32) < fim_threshold, and then SPM
 * iff (r & 0xFFFFFFFF) < spm_threshold, else PSM; mode = 0 (left alone), 1 (PSM), 2 (SPM).  With n units in the document x =
 * rnd(Kd, 0x62, 0) % (n + 1), y = rnd(Kd, 0x62, 1) % (n + 1), a = min(x, y), b = max(x, y): prefix = units [0, a), middle = [a,
 * b), suffix = [b, n); a document left alone has a = b = n.  No draw reads the batch, the row length or another document.
 * Units are ids (yabpe_fim without YABPE_FIM_PIECES) or code points of the text (yabpe_fim_cuts).
 * The cut to max_len (0: none): with X = 3 + (1 with YABPE_FIM_EOT) and C = max_len - X, the excess max(0, p + m + s - C) of a
 * transformed document leaves from the end of the suffix, then from the start of the prefix, then from the end of the middle;
 * the sentinels always survive.  A document left alone keeps its first max_len ids.  Labels: the id of every slot; with
 * YABPE_FIM_LOSS_MIDDLE `ignore` everywhere but on the middle's ids and the eot of a transformed document (every slot of a
 * document left alone keeps its label).
 *
 * yabpe_fim_cuts makes the character-level cuts: text (host or device memory) with n_docs document starts as yabpe_encode
 * takes them; per document n = its bytes that are no continuation bytes, the draws above, and the byte of its a-th and b-th
 * code point.  *out_dev_piece_off: u64[3 * n_docs], the absolute byte starts of (document, middle, suffix) -- ascending, so
 * yabpe_encode takes them (copied to the host) as the starts of 3 * n_docs documents; *out_dev_cuts: u64[3 * n_docs], (mode,
 * a, b) in characters.  UTF-8 is not validated here: the encode behind it does.  Only seed, first_doc, the two thresholds and
 * flags of *fim are read.
 *
 * yabpe_fim rearranges ragged ids.  ids / doc_off as yabpe_mask takes them, host or device memory.  Without
 * YABPE_FIM_PIECES: n_docs documents, mode and cuts drawn on token indices, cuts must be NULL.  With YABPE_FIM_PIECES:
 * n_docs is a multiple of 3, documents 3d, 3d + 1, 3d + 2 are prefix, middle and suffix of output document d (their lengths
 * in ids are p, m, s), and cuts is what yabpe_fim_cuts returned (host or device memory; only the mode is read, a mode
 * other than 1 and 2 is 0; first_doc + d then numbers nothing: no draw is made).  A document left alone is the three pieces
 * back to back.  Results: *out_dev_ids and *out_dev_labels, u32[*out_n_out] each; *out_dev_off, u64[n_out_docs + 1] with
 * n_out_docs = n_docs (n_docs / 3 with pieces) -- what the layout calls take as ids and doc_off; *out_dev_info, 4 u32 per
 * output document: (mode, p, m, s) after the cut (of a document left alone at token level: (0, kept ids, 0, 0)).
 *
 * All results are device memory owned by the library, in buffers of their own: a later encode, mask, span or layout call
 * leaves them valid.  Those of yabpe_fim_cuts live until the next yabpe_fim_cuts, those of yabpe_fim until the next
 * yabpe_fim; yabpe_fim_free and yabpe_destroy release both.
 * YABPE_E_INVALID: a threshold above 2^32, 0 < max_len <= X, an unknown flag, n_docs % 3 != 0 or cuts NULL with
 * YABPE_FIM_PIECES, cuts given without it, a doc_off that does not ascend from 0 inside the ids / the text.
 * YABPE_E_CAPACITY: a document of more than 2^32 - 1 ids, more than 2^36 output slots (judged by n_ids + X * n_out_docs, what
 * the rule can give at most).  Every error is found before a buffer is allocated. */
#define YABPE_FIM_EOT 0x1u           /* a transformed document ends with eot_id */
#define YABPE_FIM_LOSS_MIDDLE 0x2u   /* only the middle and the eot of a transformed document carry labels */
#define YABPE_FIM_PIECES 0x4u        /* the documents are the separately encoded pieces of yabpe_fim_cuts, three per document */
typedef struct yabpe_fim_t {
    uint64_t seed, first_doc;
    uint64_t fim_threshold;          /* Tf, <= 2^32 */
    uint64_t spm_threshold;          /* Ts, <= 2^32 */
    uint32_t pre_id, suf_id, mid_id, eot_id;
    uint32_t ignore;                 /* the label of a slot the loss skips */
    uint64_t max_len;                /* 0: no cut; else above X */
    uint32_t flags;                  /* YABPE_FIM_* */
} yabpe_fim_t;
int yabpe_fim_cuts(yabpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, const yabpe_fim_t *fim,
                   uint64_t **out_dev_piece_off, uint64_t **out_dev_cuts);
int yabpe_fim(yabpe_ctx *ctx, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *cuts,
              const yabpe_fim_t *fim, uint32_t **out_dev_ids, uint32_t **out_dev_labels, uint64_t **out_dev_off, uint32_t **out_dev_info,
              uint64_t *out_n_out);
int yabpe_fim_free(yabpe_ctx *ctx);
/* What the last yabpe_fim saw and drew, and its device time; cuts_ms is that of the last yabpe_fim_cuts (which also sets
 * n_docs and total_ms, and clears the rest). */
typedef struct yabpe_fim_stats_t {
    uint64_t n_docs;             /* documents that went out */
    uint64_t n_psm, n_spm;       /* transformed documents of either order */
    uint64_t n_truncated_docs;   /* documents that lost ids to max_len */
    uint64_t n_ids_dropped;      /* the ids they lost */
    uint64_t n_out;              /* output slots, sentinels included */
    double cuts_ms;              /* yabpe_fim_cuts: lead-byte table, draws and selects */
    double plan_ms;              /* the per-document plan and the scan of the lengths */
    double write_ms;             /* the output pass (with the read-back of the total and the allocation in front of it) */
    double total_ms;             /* first to last event of the last call */
} yabpe_fim_stats_t;
int yabpe_fim_stats(yabpe_ctx *ctx, yabpe_fim_stats_t *out);

/* Multi-GPU (one process per GPU; words are sharded by the caller) -----------------
 * Every rank holds its shard of the words and a replica of the pair table.  After each apply pass the ranks
 * exchange their aggregated (pair, delta) records with ONE all-gather on the compute stream and every rank adds all
 * of them to its replica (integer sums: order-independent, so all ranks select the same merge).
 * Attach the communicator after yabpe_create / yabpe_set_vocab and BEFORE yabpe_load_words; then every rank calls
 * yabpe_load_words (its shard: word_off may point into the middle of a larger offsets array) and yabpe_train
 * collectively with the same arguments.  All ranks return the same merges.
 * unique_id: the 128-byte ncclUniqueId made by yabpe_comm_unique_id on rank 0 and broadcast by the caller. */
int yabpe_comm_unique_id(uint8_t out_id[128]);
int yabpe_comm_init(yabpe_ctx *ctx, int rank, int n_ranks, const uint8_t unique_id[128]);
/* Same protocol over a caller-supplied transport instead of RCCL (other fabrics; the repo's tests use it to run
 * 2 ranks on one GPU).  fn must gather `nbytes` from every rank's DEVICE buffer send_dev into recv_dev (rank
 * order) and return 0; it is called with the context's stream idle. */
typedef int (*yabpe_allgather_fn)(void *user, const void *send_dev, void *recv_dev, uint64_t nbytes);
int yabpe_comm_init_custom(yabpe_ctx *ctx, int rank, int n_ranks, yabpe_allgather_fn fn, void *user);
/* Peer-to-peer exchange instead of the all-gather (after yabpe_comm_init / yabpe_comm_init_custom, before yabpe_load_words;
 * collective: every rank calls it).  Each rank exports its receive area as a hipIpc handle (the attached transport carries
 * the 64-byte handles once), maps its peers' areas, and from then on every exchange is ONE small launch that pushes this
 * rank's records into the peers' memory (xGMI between GPUs of a node; two processes on one GPU work the same way), raises a
 * flag there and waits for the peers' flags -- no collective kernel, no host in the loop.  The transport stays attached
 * for the rare small agreements (lockstep check, buffer growth).  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the host
 * driver only supports dmabuf IPC. */
int yabpe_comm_enable_p2p(yabpe_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* YABPE_H */
