// yabpe.hip -- C ABI (include/yabpe.h) over the HIP kernels in yabpe_kernels.h / yabpe_aux_kernels.h.
// Built only for gfx950:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC yabpe.hip -o libyabpe.so
//
// Host control flow of yabpe_train (reference trainer.py:238-300): per merge the host enqueues ONE launch on one stream
// with NO host round trip -- k_apply (streaming phase) or k_scan_skip (sparse phase) applies the merge that DevState names
// and its last workgroup selects the next one (fused_select_tail); every kernel reads the current merge / stop flags from
// DevState in HBM.  The host looks at DevState every `check_interval` merges to stop early (done), to service a halt, to
// grow the pair table, to refresh signatures / the candidate list and to retile the shrinking token stream.
// Multi-GPU: apply launch (updates leave as records) -> one all-gather -> k_delta_apply (+ the selection).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is dlopen()ed when yabpe_comm_* is first used

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/yabpe.h"
#include "yabpe_kernels.h"
#include "yabpe_aux_kernels.h"
#include "yabpe_devmem.h"
#include "yabpe_pretok_kernels.h"
#include "yabpe_encode_kernels.h"
#include "yabpe_dropout_kernels.h"
#include "yabpe_decode_kernels.h"
#include "yabpe_layout_kernels.h"
#include "yabpe_fit_kernels.h"
#include "yabpe_mask_kernels.h"
#include "yabpe_span_kernels.h"
#include "yabpe_fim_kernels.h"
#include "yabpe_replay_kernels.h"
#include "yabpe_pool_kernels.h"
#include "yabpe_norm_kernels.h"
#include "yabpe_utf8_kernels.h"
#include "yabpe_case_kernels.h"
#include "yabpe_id32_kernels.h"
#include "unicode_classes.inc"
#include "unicode_subclasses.inc"
#include "unicode_norm.inc"
#include "unicode_case.inc"

using namespace yb;

namespace {

struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl *rccl() {
    static Rccl r;
    static bool tried = false;
    if (!tried) {
        tried = true;
        // A process can hold two ROCm stacks (the system one and the copy bundled with PyTorch).  RCCL must be the
        // one that sits next to the HIP runtime THIS library is bound to, or it will not see our device.
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash);
                names.push_back(dir + "/librccl.so.1");
                names.push_back(dir + "/librccl.so");
            }
        }
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
        for (const auto &name : names) {
            r.h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (r.h) break;
        }
        if (r.h) {
            r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.h, "ncclGetUniqueId");
            r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.h, "ncclCommInitRank");
            r.AllGather = (decltype(r.AllGather))dlsym(r.h, "ncclAllGather");
            r.AllReduce = (decltype(r.AllReduce))dlsym(r.h, "ncclAllReduce");
            r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.h, "ncclCommDestroy");
            r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.h, "ncclGetErrorString");
            if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.AllReduce || !r.CommDestroy) r.h = nullptr;
        }
    }
    return r.h ? &r : nullptr;
}

// (MAX_APPLY_BLOCKS, MAX_LISTS: train_rules.h)
// blk_read: [0, MAX_LISTS) tiles read, [MAX_LISTS, 2 MAX_LISTS) second-round pieces taken, then the piece counter's own 128-B line
constexpr uint32_t BLK_READ_WORDS = 2 * MAX_LISTS + 16;
thread_local std::string g_create_error;

struct EventPair {
    hipEvent_t e0, e1, e2;  // before the apply phase, after its streaming kernel, after its last kernel
    uint32_t iter_rel;
    bool split;
};

// The slots of yabpe_ctx::lay_buf, u32 arrays unless said otherwise.  yabpe_layout_pad: ROWS, ROW_DOC (the kept lengths);
// yabpe_layout_pack: ROWS, ROW_DOC, ROW_START (ids, doc, pos: a slot each); yabpe_layout_windows: ROWS .. ROW_LEN, SPANS;
// yabpe_layout_pairs: all seven (ROW_DOC = row_pair, ROW_LEN = first_len); yabpe_layout_fit: ROWS, ROW_DOC, ROW_START (ids, doc,
// pos: a slot each) and ROW_LEN (used).
enum LayBuf {
    LB_ROWS,        // the ids of every output slot
    LB_ROW_DOC,     // per row: the document (pair) it comes from
    LB_ROW_START,   // per row: the index in its document (second side) of its first content id
    LB_ROW_LEN,     // per row: the slots it fills (pairs: the ids it keeps of the first side)
    LB_SPANS,       // with spans: a (start, end) u64 pair per output slot
    LB_SECOND_LEN,  // per row: the ids it keeps of the second side
    LB_TYPES,       // a byte per output slot
    LB_COUNT
};

}  // namespace

constexpr double CAND_MARGIN_FIRST = 0.2;  // the candidate list's margin at the start of every job (job_reset)

struct yabpe_ctx {
    int device = 0;
    int n_cu = 256;
    int apply_occ = 4;  // workgroups of the streaming-phase kernels that one CU holds at a time (asked of the runtime at creation)
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, int64_t> opt;

    // vocab
    bool have_vocab = false;
    uint32_t base_tokens = 0;
    TokTable tt{};
    // corpus
    bool have_words = false;
    bool weighted = false;
    uint64_t n_words = 0, n_words_input = 0, tokens_initial = 0;
    uint32_t n_tiles = 0;
    uint16_t *tiles = nullptr, *tiles_alt = nullptr;
    uint32_t tiles_cap = 0, tiles_alt_cap = 0;  // capacities in tiles
    uint32_t *tile_len = nullptr, *tile_len_alt = nullptr;
    uint32_t *tile_wbase = nullptr, *tile_wbase_alt = nullptr;
    uint32_t *wfreq = nullptr;
    // long words
    uint32_t n_long = 0;
    uint16_t *long_tok = nullptr;
    unsigned long long *long_sig = nullptr;  // one blocked-Bloom signature per long word (k_apply_long launches only what may hold the pair)
    uint32_t long_sig_stride = 0;
    unsigned long long *long_off = nullptr;
    uint32_t *long_len = nullptr, *long_freq = nullptr;
    uint64_t long_tokens = 0;
    // pair table
    PairTable table{};
    uint64_t table_cap = 0;
    // state
    DevState *st = nullptr;
    DevState *st_host = nullptr;  // pinned
    Best *partials = nullptr;
    uint32_t n_partials = 0, n_partials_cap = 0;
    // records of the last train call
    uint32_t rec_cap = 0, rec_n = 0;
    uint32_t *rec_left = nullptr, *rec_right = nullptr, *rec_merged = nullptr;
    unsigned long long *rec_count = nullptr, *rec_sites = nullptr, *rec_live = nullptr;
    std::vector<uint64_t> log_sites, log_live;
    std::vector<uint32_t> ev_iter;
    std::vector<float> ev_us;
    // stats
    yabpe_stats_t stats{};
    std::vector<EventPair> events;
    // synth buffers
    std::vector<void *> synth_bufs;
    std::vector<void *> pretok_bufs;          // staged text / word offsets handed out by yabpe_pretokenize
    uint8_t *pt_cls = nullptr;                // class per code point (unicode_classes.inc expanded), built on first use
    uint8_t *pt_cls5 = nullptr;               // the o200k_base pattern's table (pt5_table_entry), built on its first use
    // normaliser (yabpe_normalize): the tables of unicode_norm.inc, built on first use, and the results of the last call
    uint16_t *nfc_prop = nullptr;
    uint32_t *nfc_decomp = nullptr, *nfc_pairs = nullptr;
    std::vector<void *> norm_bufs;
    yabpe_normalize_stats_t norm_stats{};
    hipEvent_t norm_ev[5] = {};
    // invalid UTF-8 replaced or dropped (yabpe_utf8_repair): the results of the last call
    std::vector<void *> utf8_bufs;
    yabpe_utf8_stats_t utf8_stats{};
    hipEvent_t utf8_ev[3] = {};
    // lower-casing (yabpe_lowercase): the table of unicode_case.inc, built on first use, and the results of the last call
    uint32_t *case_tab = nullptr;
    std::vector<void *> case_bufs;
    yabpe_lowercase_stats_t case_stats{};
    hipEvent_t case_ev[4] = {};
    // encoder (yabpe_encode_set_model / yabpe_encode)
    bool have_enc_model = false;
    unsigned long long *enc_keys = nullptr;   // pair table: (a << 32 | b) -> enc_vals (rank, result)
    uint32_t *enc_vals = nullptr;
    unsigned long long enc_mask = 0;
    uint32_t *enc_out_id = nullptr;           // internal id -> output id
    uint8_t *enc_sp_bytes = nullptr, *enc_sp_has = nullptr;
    uint32_t *enc_sp_off = nullptr, *enc_sp_id = nullptr;
    uint32_t enc_n_special = 0, enc_sp_max_len = 0;
    uint32_t *enc_ids = nullptr;              // results of the last yabpe_encode / yabpe_encode_spans
    unsigned long long *enc_doc = nullptr;
    unsigned long long *enc_spans = nullptr;  // (yabpe_encode_spans only)
    uint32_t *enc_words = nullptr;            // (yabpe_encode_words only)
    yabpe_encode_stats_t enc_stats{};
    unsigned long long enc_sums[4] = {0, 0, 0, 0};  // checksum, words, tokens, specials taken
    bool enc_done = false;
    hipEvent_t enc_ev[8] = {};
    // decoder (yabpe_decode_set_model / yabpe_decode)
    bool have_dec_model = false;
    uint2 *dec_ent = nullptr;                 // id -> (offset into dec_pool, length)
    uint8_t *dec_pool = nullptr;
    uint32_t dec_n = 0;                       // ids in the table
    uint8_t *dec_text = nullptr;              // results of the last yabpe_decode
    unsigned long long *dec_doc = nullptr;
    yabpe_decode_stats_t dec_stats{};
    hipEvent_t dec_ev[7] = {};
    // fixed-shape batches (yabpe_layout_pad / yabpe_layout_pack / yabpe_layout_windows / yabpe_layout_pairs)
    uint32_t *lay_buf[LB_COUNT] = {};         // results of the last layout call, by LayBuf (which says what each call keeps where)
    yabpe_layout_stats_t lay_stats{};
    hipEvent_t lay_ev[4] = {};
    // masked-language-model batches (yabpe_mask): the results of the last call
    uint32_t *mask_ids = nullptr, *mask_labels = nullptr;
    yabpe_mask_stats_t mask_stats{};
    hipEvent_t mask_ev[4] = {};
    // span-corruption batches (yabpe_span_corrupt): the results of the last call
    uint32_t *span_in = nullptr, *span_tgt = nullptr;
    unsigned long long *span_in_off = nullptr, *span_tgt_off = nullptr;
    yabpe_span_stats_t span_stats{};
    hipEvent_t span_ev[6] = {};
    // fill-in-the-middle batches: the results of the last yabpe_fim_cuts ([0..1]) and of the last yabpe_fim ([2..5])
    void *fim_buf[6] = {};
    yabpe_fim_stats_t fim_stats{};
    hipEvent_t fim_ev[4] = {};
    // resumed load (yabpe_load_words_resumed)
    yabpe_resume_stats_t resume_stats{};
    // persistent word pool (yabpe_pool_add / yabpe_pool_get): arena, off / count / hash, slots (pool_logic.h)
    bool have_pool = false;
    PoolView wpool{};
    uint64_t wpool_arena_cap = 0, wpool_n = 0, wpool_bytes = 0;
    yabpe_pool_stats_t wpool_stats{};
    hipEvent_t wpool_ev[4] = {};
    // misc device scratch
    unsigned long long *scratch64 = nullptr;  // 16 x u64: [0] live sum [1] freq overflow [2,3] long words [4,5,6] verify/checksum
                                              // [7] comm_max [8] exchange record count [9] local count-table entries [10..12] comm_max3
    unsigned long long *blk_stats = nullptr;  // 2 x MAX_APPLY_BLOCKS per-workgroup counters of k_apply
    uint32_t blk_used = 0;                    // largest grid that wrote blk_stats since they were last folded
    bool split_mode = false;         // the sparse form (skip index + batches of merges per launch) instead of the streaming one
    uint32_t kmax_now = 1;           // DevState::kmax as last written
    std::vector<float> ev_scan_us;
    // skip index
    unsigned long long *sig = nullptr;
    uint32_t sig_stride = 0;
    unsigned long long *blk_read = nullptr;  // [BLK_READ_WORDS] tiles read by k_scan_skip, accumulated; pieces taken; the piece counter
    uint64_t scan_skip_launches = 0;
    uint64_t piece_tag = 0;                  // tag of the last launch that used the piece counter: never reset while blk_read lives
    bool sig_valid = false;
    uint32_t sig_built_at = 0;
    uint64_t sig_tokens_at_build = 0;  // T when the signatures were last built (stale bits grow with the sites merged since)
    uint64_t sig_builds = 0;
    // candidate argmax
    CandState *cand_state = nullptr;
    uint32_t cand_built_at = 0;      // merge index (of this yabpe_train call) at which cand[] was last rebuilt
    unsigned long long cand_best_at_build = 0;
    uint32_t *sel_ticket = nullptr;  // finished-workgroup counters (TICKET_WORDS; the last workgroup selects; they reset themselves)
    unsigned long long *cand = nullptr;
    unsigned long long *cand_bits = nullptr;  // "listed" bit per slot of c->table (written whole by every k_cand_rebuild)
    uint64_t cand_bits_cap = 0;               // table capacity it was sized to
    bool use_cand = false;
    uint64_t cand_rebuilds = 0, cand_rescans = 0;
    double cand_margin = CAND_MARGIN_FIRST;  // T = best count x (1 - margin); adapted so that the list stays short
    uint32_t cand_n_at_build = 0;
    // fused per-merge launch: the apply kernel of merge i ends with the selection of merge i + 1
    bool pending = false;            // a merge has been selected (recorded) and not applied yet
    uint64_t fused_launches = 0;
    // multi-GPU
    int rank = 0, n_ranks = 1;
    bool multi = false;  // exchange path active (n_ranks > 1, or a 1-rank communicator forced for testing)
    ncclComm_t comm = nullptr;
    yabpe_allgather_fn ag_fn = nullptr;  // custom transport (tests / other fabrics) instead of RCCL
    void *ag_user = nullptr;
    unsigned long long *xsmall = nullptr;  // n_ranks x u64 receive slots for small agreements
    uint8_t *xsend = nullptr, *xrecv = nullptr;  // [DeltaHdr | xcap DeltaRec] of this rank / of every rank
    uint64_t exchange_growths = 0;  // times the exchange buffers had to grow (a merge produced more records than fit)
    uint64_t exchange_max_records = 0;  // largest record count of one rank seen at a batch end
    uint32_t xcap = 0;      // records per rank the exchange buffers hold
    uint64_t xstride = 0;   // bytes per rank buffer
    uint32_t xeff = 0;      // records per rank an exchange TRANSMITS (<= xcap): follows what the merges really produce, so
                            // that an all-gather moves a few dozen KiB per rank late in a job, not the whole 256 KiB buffer
    uint64_t xeff_sum = 0;  // (statistics: sum of xeff over the exchanges)
    uint32_t xseen[4] = {0, 0, 0, 0};  // the largest record counts of the last four batches
    uint64_t exchanges = 0;
    // peer-to-peer exchange (yabpe_comm_enable_p2p): receive areas mapped through hipIpc handles
    bool p2p = false;
    uint8_t *p2p_area = nullptr;               // this rank's receive area: 2 halves of n_ranks slots + the flag words (plain hipMalloc: exported)
    std::vector<uint8_t *> p2p_peer;           // every rank's area as mapped here (own rank: p2p_area)
    uint64_t p2p_half = 0, p2p_flags_off = 0, p2p_seq = 0, p2p_stride = 0;  // p2p_stride: bytes of one sender's slot in an area
    uint32_t p2p_cap = 0;                      // records a slot holds (fixed for the job: the areas are mapped once)
    hipEvent_t p2p_e0 = nullptr, p2p_e1 = nullptr;  // (statistics: every 64th exchange is timed)
    bool p2p_pending = false;                  // an event pair was recorded and not read yet
    // u32-id merge loop (option "id_bits" = 32): its own stream, long-word buffer and pair table; tile_len,
    // tile_wbase, wfreq, long_off / long_len / long_freq, the token table and the state are the fields above
    int id_bits = 16;
    bool id_bits_fixed = false;                // yabpe_set_vocab has read the option
    uint32_t *tiles32 = nullptr, *tiles32_alt = nullptr, *long_tok32 = nullptr;
    uint32_t tiles32_alt_cap = 0;
    PairTable32 table32{};
    Best32 *partials32 = nullptr;
    uint32_t tok_cap32 = 0;                    // ids the token arrays hold
    uint64_t pool_growths32 = 0;
    Cand32 *cand32_state = nullptr;            // candidate list of the u32 selection (tables of "cand_min_slots" slots or more)
    uint32_t *cand32_list = nullptr;
    uint32_t cand32_cap = 0;
};

namespace {

int fail(yabpe_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c)
        c->err = buf;
    else
        g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fail((c), YABPE_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

#define NCCLCHK(c, call)                                                                            \
    do {                                                                                           \
        ncclResult_t r__ = (call);                                                                 \
        if (r__ != ncclSuccess)                                                                    \
            return fail((c), YABPE_E_COMM, "%s failed: %s (%s:%d)", #call,                         \
                        rccl() && rccl()->GetErrorString ? rccl()->GetErrorString(r__) : "?", __FILE__, __LINE__); \
    } while (0)

// Device memory comes from the block cache of yabpe_devmem.h; these two add the context's error text.
template <class T>
int dmalloc(yabpe_ctx *c, T **p, uint64_t n) {
    HIPCHK(c, dev_alloc(c ? c->device : 0, c ? c->rank : -1, (void **)p, n * sizeof(T)));
    return 0;
}
#define TRY(x)               \
    do {                     \
        int r__ = (x);       \
        if (r__ != 0) return r__; \
    } while (0)

void dfree(void *p) { dev_free(p); }

int64_t optv(yabpe_ctx *c, const char *k, int64_t dflt) {
    auto it = c->opt.find(k);
    return it == c->opt.end() ? dflt : it->second;
}

bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

inline uint32_t cdiv64(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

int fill_u16(yabpe_ctx *c, uint16_t *p, uint64_t n, uint16_t v) {
    if (!n) return 0;
    uint64_t th = (n + 7) / 8;
    hipLaunchKernelGGL(k_fill_u16, dim3(cdiv64(th, 256)), dim3(256), 0, c->stream, p, (unsigned long long)n, v);
    HIPCHK(c, hipGetLastError());
    return 0;
}
int fill_u32(yabpe_ctx *c, uint32_t *p, uint64_t n, uint32_t v) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_fill_u32, dim3(cdiv64(n, 256)), dim3(256), 0, c->stream, p, (unsigned long long)n, v);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int state_pull(yabpe_ctx *c) {
    HIPCHK(c, hipMemcpyAsync(c->st_host, c->st, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int state_push(yabpe_ctx *c) {
    HIPCHK(c, hipMemcpyAsync(c->st, c->st_host, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------- pair table
void table_free(PairTable &t) {
    dfree(t.keys);
    dfree(t.cnt);
    t.keys = nullptr;
    t.cnt = nullptr;
    t.cand_cs = nullptr;
    t.cand_list = nullptr;
    t.cand_bits = nullptr;
    t.cand_T = 0;
    t.sink_rec = nullptr;
    t.sink_hdr = nullptr;
    t.sink_cap = 0;
}

int table_alloc(yabpe_ctx *c, PairTable &t, uint64_t cap, unsigned long long *entries_ctr) {
    TRY(dmalloc(c, &t.keys, cap));
    TRY(dmalloc(c, &t.cnt, cap));
    t.cap = (uint32_t)cap;
    // (multi-GPU: a replica must never give up on a probe chain on its own -- its layout differs from its peers' -- so the
    //  chain may run over the whole table; the deterministic 80 % rule of the selection stops all ranks long before that)
    t.max_probe = c->multi ? (uint32_t)cap : (uint32_t)std::min<uint64_t>(cap, 2048);
    t.sink_rec = nullptr;
    t.sink_hdr = nullptr;
    t.sink_cap = 0;
    t.entries = entries_ctr;
    // (the candidate list is attached to the main table only, once it is built: cand_attach / cand_rebuild)
    t.cand_cs = nullptr;
    t.cand_list = nullptr;
    t.cand_bits = nullptr;
    t.cand_T = 0;
    HIPCHK(c, hipMemsetAsync(t.keys, 0xFF, cap * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(t.cnt, 0, cap * sizeof(unsigned long long), c->stream));
    return 0;
}

// The main table has new slots (rebuilt, grown): the candidate list is detached and its "listed" bitmap, which names slots,
// goes with it; the caller's next check rebuilds both (cand_rebuild) at the new capacity.
int cand_attach(yabpe_ctx *c) {
    c->use_cand = false;
    PairTable &t = c->table;
    t.cand_cs = nullptr;
    t.cand_list = nullptr;
    t.cand_bits = nullptr;
    dfree(c->cand_bits);
    c->cand_bits = nullptr;
    c->cand_bits_cap = 0;
    if (!optv(c, "cand_argmax", 1)) return 0;
    if (!c->sel_ticket) {
        TRY(dmalloc(c, &c->sel_ticket, TICKET_WORDS));
        HIPCHK(c, hipMemsetAsync(c->sel_ticket, 0, TICKET_WORDS * 4, c->stream));
    }
    if (!c->cand_state) {
        TRY(dmalloc(c, &c->cand_state, 1));
        TRY(dmalloc(c, &c->cand, CAND_CAP));
    }
    return 0;
}

// list = every slot with count >= T, T = best_count x (1 - margin); enables the candidate argmax from here on.  While the
// list is attached to c->table, every kernel that raises a count appends to it (cand_note), so it stays exact for as long
// as the maximum stays >= T.  The margin adapts: the fused selection is ONE workgroup reading the whole list.
int cand_rebuild(yabpe_ctx *c, unsigned long long best_count) {
    c->use_cand = false;
    c->table.cand_cs = nullptr;
    c->table.cand_list = nullptr;
    c->table.cand_bits = nullptr;
    if (!optv(c, "cand_argmax", 1) || !c->cand_state || best_count < (unsigned long long)optv(c, "cand_min_count", 16)) return 0;
    if (!c->cand_bits || c->cand_bits_cap != c->table.cap) {  // (k_cand_rebuild writes every word: nothing to clear)
        dfree(c->cand_bits);
        c->cand_bits = nullptr;
        c->cand_bits_cap = 0;
        TRY(dmalloc(c, &c->cand_bits, yb_cand_bitmap_words(c->table.cap)));
        c->cand_bits_cap = c->table.cap;
    }
    const uint32_t target = (uint32_t)std::max<int64_t>(64, optv(c, "cand_target", 768));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, c->table_cap / (BLOCK * 8)));
    CandState h{};
    for (int attempt = 0; attempt < 12; ++attempt) {
        unsigned long long margin = (unsigned long long)((double)best_count * c->cand_margin);
        if (margin < 1) margin = 1;
        h = CandState{best_count - std::min(margin, best_count - 1), 0u, 0u, 0u, 0u};
        HIPCHK(c, hipMemcpyAsync(c->cand_state, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
        PairTable t = c->table;
        t.cand_list = c->cand;
        t.cand_bits = c->cand_bits;
        t.cand_cs = c->cand_state;
        t.cand_T = h.T;
        {
            CandParams P{t, c->tt.rec, c->partials, c->st, c->cand_state, nullptr, SelectParams{}};
            hipLaunchKernelGGL(k_cand_rebuild, dim3(grid), dim3(BLOCK), 0, c->stream, P);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&h, c->cand_state, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->cand_rebuilds++;
        if ((h.overflow || h.n > target) && margin > 1) { // too many pairs that close to the top: halve the margin, again
            c->cand_margin *= 0.5;
            continue;
        }
        break;
    }
    // room to spare: rebuild less often next time -- and a batch can reach further down (early in a job the best counts lie
    // far apart: a selection can only batch pairs that are on the list)
    if (h.n < target / 8) c->cand_margin = std::min((double)optv(c, "cand_margin_max_pct", 60) / 100.0, c->cand_margin * 2.0);
    c->use_cand = !h.overflow && h.n < CAND_CAP / 2;
    c->cand_n_at_build = h.n;
    if (c->use_cand) {
        c->table.cand_cs = c->cand_state;
        c->table.cand_list = c->cand;
        c->table.cand_bits = c->cand_bits;
        c->table.cand_T = h.T;
    }
    return 0;
}

uint32_t count_grid(yabpe_ctx *c) {
    return count_grid_rule(c->n_tiles, (uint32_t)c->n_cu, (uint32_t)c->apply_occ, optv(c, "apply_blocks", OPT_UNSET));
}

int fold_stats(yabpe_ctx *c) {
    FoldParams F{c->st, c->blk_stats, std::max(c->blk_used, 1u)};
    hipLaunchKernelGGL(k_fold_stats, dim3(1), dim3(BLOCK), 0, c->stream, F);
    HIPCHK(c, hipGetLastError());
    c->blk_used = 0;
    return 0;
}

// THE collective: every rank contributes `nbytes` from device memory, every rank receives all contributions in
// rank order.  RCCL all-gather on the compute stream (asynchronous), or the caller's transport (synchronous).
int comm_allgather(yabpe_ctx *c, const void *send, void *recv, uint64_t nbytes) {
    if (c->comm) {
        NCCLCHK(c, rccl()->AllGather(send, recv, nbytes, ncclUint8, c->comm, c->stream));
        return 0;
    }
    if (!c->ag_fn) return fail(c, YABPE_E_COMM, "no transport attached");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = c->ag_fn(c->ag_user, send, recv, nbytes);
    if (rc != 0) return fail(c, YABPE_E_COMM, "custom all-gather transport failed (%d)", rc);
    return 0;
}

int comm_max(yabpe_ctx *c, unsigned long long v, unsigned long long *out);

// All ranks: dump the local table `lt` as records, all-gather them (padded to the largest rank), add every rank's
// records into `t`.  Used for counts that cannot use the dense byte histogram (weighted words, recounts).
int exchange_table(yabpe_ctx *c, PairTable lt, uint64_t lcap, PairTable t) {
    unsigned long long *d_cnt = &c->scratch64[8];
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 8, c->stream));
    // first pass only counts (cap 0), so that every rank learns the padded size
    const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, lcap / BLOCK));
    DumpParams D0{lt, nullptr, d_cnt, 0};
    hipLaunchKernelGGL(k_table_dump, dim3(grid), dim3(BLOCK), 0, c->stream, D0);
    HIPCHK(c, hipGetLastError());
    unsigned long long mine = 0, maxn = 0;
    HIPCHK(c, hipMemcpyAsync(&mine, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    TRY(comm_max(c, mine, &maxn));
    if (maxn == 0) return 0;
    uint8_t *send = nullptr, *recv = nullptr;
    const uint64_t stride = 16 + maxn * sizeof(DeltaRec);
    TRY(dmalloc(c, &send, stride));
    TRY(dmalloc(c, &recv, stride * c->n_ranks));
    HIPCHK(c, hipMemsetAsync(send, 0, 16, c->stream));
    DumpParams D1{lt, reinterpret_cast<DeltaRec *>(send + 16), reinterpret_cast<unsigned long long *>(send), maxn};
    hipLaunchKernelGGL(k_table_dump, dim3(grid), dim3(BLOCK), 0, c->stream, D1);
    HIPCHK(c, hipGetLastError());
    TRY(comm_allgather(c, send, recv, stride));
    std::vector<unsigned long long> counts(c->n_ranks);
    for (int r = 0; r < c->n_ranks; ++r)
        HIPCHK(c, hipMemcpyAsync(&counts[r], recv + (uint64_t)r * stride, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->n_ranks; ++r) {
        if (!counts[r]) continue;
        RecApplyParams A{reinterpret_cast<const DeltaRec *>(recv + (uint64_t)r * stride + 16), counts[r], t, c->st};
        hipLaunchKernelGGL(k_records_apply, dim3(cdiv64(counts[r], BLOCK)), dim3(BLOCK), 0, c->stream, A);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(send);
    dfree(recv);
    return 0;
}

// max over ranks of a small integer (host-visible); identity on one GPU
int comm_max(yabpe_ctx *c, unsigned long long v, unsigned long long *out) {
    *out = v;
    if (!c->multi) return 0;
    HIPCHK(c, hipMemcpyAsync(&c->scratch64[7], &v, 8, hipMemcpyHostToDevice, c->stream));
    TRY(comm_allgather(c, &c->scratch64[7], c->xsmall, 8));
    std::vector<unsigned long long> all(c->n_ranks);
    HIPCHK(c, hipMemcpyAsync(all.data(), c->xsmall, 8 * (size_t)c->n_ranks, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto x : all) *out = std::max(*out, x);
    return 0;
}

// max over ranks of three small integers in ONE exchange (host-visible); identity on one GPU
int comm_max3(yabpe_ctx *c, unsigned long long v[3]) {
    if (!c->multi) return 0;
    HIPCHK(c, hipMemcpyAsync(&c->scratch64[10], v, 24, hipMemcpyHostToDevice, c->stream));
    TRY(comm_allgather(c, &c->scratch64[10], c->xsmall, 24));
    std::vector<unsigned long long> all(3 * (size_t)c->n_ranks);
    HIPCHK(c, hipMemcpyAsync(all.data(), c->xsmall, 24 * (size_t)c->n_ranks, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->n_ranks; ++r)
        for (int k = 0; k < 3; ++k) v[k] = std::max(v[k], all[3 * (size_t)r + k]);
    return 0;
}

// pair counts of THIS rank's shard into `t` (zeroed by the caller), generic tokens
int launch_count_local(yabpe_ctx *c, PairTable t) {
    if (c->n_tiles) {
        CountParams P{c->tiles, c->tile_len, c->tile_wbase, c->wfreq, c->n_tiles, t, c->st};
        if (c->weighted)
            hipLaunchKernelGGL(k_count<true>, dim3(count_grid(c)), dim3(BLOCK), 0, c->stream, P);
        else
            hipLaunchKernelGGL(k_count<false>, dim3(count_grid(c)), dim3(BLOCK), 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
    }
    if (c->n_long) {
        LongParams L{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, t, c->st, nullptr, 0u};
        hipLaunchKernelGGL(k_count_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// Full recount of the resident stream -- of ALL ranks' shards when a communicator is attached -- into `t`
// (zeroed by the caller).  all_bytes: every token is still a byte (initial count of the flat layout).
int launch_count(yabpe_ctx *c, PairTable t, bool all_bytes = false) {
    if (all_bytes && !c->weighted && optv(c, "dense_count", 1)) {
        // trainer.py:227-235 over 256 x 256 keys: dense LDS histograms, summed across ranks by one all-reduce
        unsigned long long *dense = nullptr;
        TRY(dmalloc(c, &dense, 65536));
        HIPCHK(c, hipMemsetAsync(dense, 0, 65536 * 8, c->stream));
        if (c->n_tiles) {
            const uint32_t bpp = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(c->n_cu / 2, (c->n_tiles + CB_WAVES - 1) / CB_WAVES));
            CountBytesParams P{c->tiles, c->tile_len, c->n_tiles, dense, bpp};
            hipLaunchKernelGGL(k_count_bytes, dim3(4 * bpp), dim3(CB_BLOCK), 0, c->stream, P);
        }
        if (c->multi) {  // sum the per-rank histograms: gather all, add rows
            unsigned long long *all = nullptr;
            TRY(dmalloc(c, &all, 65536ull * c->n_ranks));
            TRY(comm_allgather(c, dense, all, 65536 * 8));
            hipLaunchKernelGGL(k_sum_rows, dim3(65536 / BLOCK), dim3(BLOCK), 0, c->stream, all, dense, 65536u, (uint32_t)c->n_ranks);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));
            dfree(all);
        }
        DenseToTableParams D{dense, t, c->st};
        hipLaunchKernelGGL(k_dense_to_table, dim3(65536 / BLOCK), dim3(BLOCK), 0, c->stream, D);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(dense);
        if (c->n_long) {  // long words of this rank (bytes too) -- their pairs go through the generic exchange
            if (!c->multi) {
                LongParams L{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, t, c->st, nullptr, 0u};
                hipLaunchKernelGGL(k_count_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, L);
                HIPCHK(c, hipGetLastError());
            }
        }
        if (!c->multi) return 0;
        // multi-GPU: any rank may hold long words; exchange their pairs generically (usually nothing)
        unsigned long long any_long = 0;
        TRY(comm_max(c, c->n_long, &any_long));
        if (!any_long) return 0;
        PairTable lt{};
        HIPCHK(c, hipMemsetAsync(&c->scratch64[9], 0, 8, c->stream));
        TRY(table_alloc(c, lt, 1ull << 18, &c->scratch64[9]));
        if (c->n_long) {
            LongParams L{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, lt, c->st, nullptr, 0u};
            hipLaunchKernelGGL(k_count_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, L);
            HIPCHK(c, hipGetLastError());
        }
        int rc = exchange_table(c, lt, 1ull << 18, t);
        table_free(lt);
        return rc;
    }
    if (!c->multi) return launch_count_local(c, t);
    // generic multi-GPU count: local table -> records -> all-gather -> sum into t
    PairTable lt{};
    const uint64_t lcap = (uint64_t)t.cap;
    HIPCHK(c, hipMemsetAsync(&c->scratch64[9], 0, 8, c->stream));
    TRY(table_alloc(c, lt, lcap, &c->scratch64[9]));
    TRY(launch_count_local(c, lt));
    int rc = exchange_table(c, lt, lcap, t);
    table_free(lt);
    return rc;
}

// (Re)build the pair table from the token stream with at least `min_cap` slots; grows until the load is <= 1/2.
int table_rebuild(yabpe_ctx *c, uint64_t min_cap, bool all_bytes = false) {
    uint64_t cap = std::max<uint64_t>(min_cap, 1ull << optv(c, "table_min_log2", 16));
    bool shrunk = false;
    for (int attempt = 0; attempt < 16; ++attempt) {
        table_free(c->table);
        HIPCHK(c, hipMemsetAsync(&c->st->table_entries, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(&c->st->halt_req, 0, sizeof(uint32_t), c->stream));
        TRY(table_alloc(c, c->table, cap, &c->st->table_entries));
        c->table_cap = cap;
        TRY(launch_count(c, c->table, all_bytes));
        TRY(state_pull(c));
        unsigned long long bad = (c->st_host->halt_req != 0 || c->st_host->table_entries * 2 > cap) ? 1 : 0, any_bad = 0;
        TRY(comm_max(c, bad, &any_bad));  // replicas differ in layout: all ranks retry together
        if (!any_bad) {
            if (!shrunk && c->st_host->table_entries * 32 < cap && cap > (1ull << 16)) {
                // far too roomy (scans of the table -- candidate rebuilds, the fallback argmax -- read every slot): count
                // once more at ~8x the entries (the entry count is the same on every rank, so all ranks take this branch together)
                shrunk = true;
                cap = std::max<uint64_t>(c->st_host->table_entries * 8, 1ull << 16);
                continue;
            }
            c->stats.table_rebuilds++;
            TRY(cand_attach(c));
            return 0;
        }
        cap *= 4;
        if (cap > (1ull << 31)) break;
    }
    return fail(c, YABPE_E_CAPACITY, "pair table does not fit (more than 2^29 distinct pairs)");
}

// Grow the pair table by re-inserting its live entries (entries whose count fell to 0 are dropped).
int table_grow(yabpe_ctx *c, uint64_t new_cap) {
    for (int attempt = 0; attempt < 8; ++attempt, new_cap = new_cap * 3 / 2) {
        PairTable nt{};
        HIPCHK(c, hipMemsetAsync(&c->st->table_entries, 0, sizeof(unsigned long long), c->stream));
        TRY(table_alloc(c, nt, new_cap, &c->st->table_entries));
        RehashParams R{c->table, nt, c->st};
        const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, std::max<uint64_t>(1, c->table_cap / BLOCK));
        hipLaunchKernelGGL(k_rehash, dim3(grid), dim3(BLOCK), 0, c->stream, R);
        HIPCHK(c, hipGetLastError());
        TRY(state_pull(c));
        if (c->st_host->halt_req == 0 && c->st_host->table_entries * 10 <= new_cap * 6) {
            table_free(c->table);
            c->table = nt;
            c->table_cap = new_cap;
            c->stats.table_rebuilds++;
            TRY(cand_attach(c));
            return 0;
        }
        table_free(nt);
        c->st_host->halt_req = 0;
        TRY(state_push(c));
    }
    return fail(c, YABPE_E_CAPACITY, "pair table does not fit");
}

#define YB_TRACE_C(c, ...) do { if (optv(c, "trace_host", 0)) { fprintf(stderr, "[yabpe r%d] ", (c)->rank); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); fflush(stderr); } } while (0)
// The peer-to-peer receive areas are exported and mapped ONCE per job, at their final size, and never freed while the job
// lives.  Taking them down and up again when the exchange buffers grow (unmap, free, allocate, export, map) does not survive
// on this runtime: about one time in five hipIpcOpenMemHandle of the re-exported area failed on one rank and never returned
// on the other (two processes, one MI355X, the 8 GiB job's second growth) -- whether the ranks map one at a time or together,
// with or without a barrier between unmapping and freeing.  A first mapping has never failed.
void p2p_close(yabpe_ctx *c) {  // (yabpe_destroy: no collective here -- a peer may be gone)
    for (size_t r = 0; r < c->p2p_peer.size(); ++r)
        if (c->p2p_peer[r] && (int)r != c->rank) (void)hipIpcCloseMemHandle(c->p2p_peer[r]);
    c->p2p_peer.clear();
    // the own area: a peer may still have it mapped -- left to the process's exit (the driver drops it with its last mapping)
    if (c->p2p_area && c->n_ranks <= 1) (void)hipFree(c->p2p_area);
    c->p2p_area = nullptr;
}

// Build the peer-to-peer receive areas: `p2p_cap` records per sender and half (option "p2p_cap_records", 4 Mi = 64 MiB per
// slot: 1 GiB of a rank's 288 GB at 8 ranks), exchange the IPC handles through the attached transport (one all-gather of
// 64 bytes per rank), map the peers' areas.  Collective: every rank calls it at the same point and runs the same sequence of
// collectives whatever fails locally; if ANY rank could not export or map a buffer, all ranks drop the peer-to-peer path
// together and keep exchanging through the transport (c->p2p = false, no error).
int p2p_setup(yabpe_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->p2p_area) return 0;  // (once)
    unsigned long long failed = 0;
    std::string why;
    if (c->n_ranks > XCHG_MAX_RANKS) { failed = 1; why = "too many ranks"; }
    c->p2p_cap = (uint32_t)std::max<int64_t>((int64_t)c->xcap, std::min<int64_t>(optv(c, "p2p_cap_records", 4ll << 20), 1ll << 28));
    c->p2p_stride = 16 + (uint64_t)c->p2p_cap * sizeof(DeltaRec);
    c->p2p_half = c->p2p_stride * (uint64_t)c->n_ranks;
    c->p2p_flags_off = (2 * c->p2p_half + 255) & ~255ull;
    const uint64_t bytes = c->p2p_flags_off + 2ull * c->n_ranks * 8 + 256;
    hipIpcMemHandle_t mine;
    memset(&mine, 0, sizeof mine);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    if (!failed) {
        YB_TRACE_C(c, "p2p setup: allocate %llu bytes", (unsigned long long)bytes);
        hipError_t e = hipMalloc((void **)&c->p2p_area, bytes);
        // (only the flag words have to start at zero: a slot is read up to the count its header announces)
        if (e == hipSuccess) e = hipMemset(c->p2p_area + c->p2p_flags_off, 0, bytes - c->p2p_flags_off);
        if (e == hipSuccess) e = hipIpcGetMemHandle(&mine, c->p2p_area);
        if (e != hipSuccess) { failed = 1; why = std::string("export: ") + hipGetErrorString(e); (void)hipGetLastError(); }
    }
    uint8_t *d_h = nullptr, *d_all = nullptr;
    TRY(dmalloc(c, &d_h, 64));
    TRY(dmalloc(c, &d_all, 64ull * c->n_ranks));
    HIPCHK(c, hipMemcpy(d_h, &mine, 64, hipMemcpyHostToDevice));
    TRY(comm_allgather(c, d_h, d_all, 64));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<hipIpcMemHandle_t> all(c->n_ranks);
    HIPCHK(c, hipMemcpy(all.data(), d_all, 64ull * c->n_ranks, hipMemcpyDeviceToHost));
    dfree(d_h);
    dfree(d_all);
    c->p2p_peer.assign(c->n_ranks, nullptr);
    for (int r = 0; r < c->n_ranks && !failed; ++r) {
        if (r == c->rank) { c->p2p_peer[r] = c->p2p_area; continue; }
        void *q = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&q, all[r], hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { failed = 1; why = std::string("map: ") + hipGetErrorString(e); (void)hipGetLastError(); break; }
        c->p2p_peer[r] = (uint8_t *)q;
    }
    c->p2p_seq = 0;
    YB_TRACE_C(c, "p2p setup: mapped (failed %llu)", failed);
    // nobody pushes before every rank has mapped everything -- and everybody learns whether somebody could not
    unsigned long long any_failed = 0;
    TRY(comm_max(c, failed, &any_failed));
    if (any_failed) {
        c->p2p = false;  // (what is mapped stays mapped until yabpe_destroy: nothing is taken down while peers may be in the runtime)
        if (failed && optv(c, "trace_exchange", 0)) fprintf(stderr, "[yabpe r%d] peer-to-peer exchange not available here (%s): exchanging through the transport\n", c->rank, why.c_str());
    }
    return 0;
}

// (re)allocate the per-iteration exchange buffers for `cap` records per rank
int comm_buffers(yabpe_ctx *c, uint32_t cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(c->xsend);
    dfree(c->xrecv);
    c->xsend = c->xrecv = nullptr;
    c->xcap = cap;
    c->xeff = cap;
    c->xstride = 16 + (uint64_t)cap * sizeof(DeltaRec);
    TRY(dmalloc(c, &c->xsend, c->xstride));
    TRY(dmalloc(c, &c->xrecv, c->xstride * c->n_ranks));
    HIPCHK(c, hipMemsetAsync(c->xsend, 0, c->xstride, c->stream));
    HIPCHK(c, hipMemsetAsync(c->xrecv, 0, c->xstride * c->n_ranks, c->stream));
    // (the peer-to-peer areas keep their size: a buffer beyond it -- the same on every rank -- goes through the transport from here on)
    if (c->p2p && c->p2p_area && cap > c->p2p_cap) {
        c->p2p = false;
        if (optv(c, "trace_exchange", 0)) fprintf(stderr, "[yabpe r%d] exchange buffers of %u records exceed the peer-to-peer areas (%u): exchanging through the transport\n", c->rank, cap, c->p2p_cap);
    }
    return 0;
}

int refresh_live_slots(yabpe_ctx *c) {
    HIPCHK(c, hipMemsetAsync(&c->scratch64[0], 0, 8, c->stream));
    if (c->n_tiles) {
        hipLaunchKernelGGL(k_sum_u32, dim3(std::min<uint32_t>(1024, cdiv64(c->n_tiles, BLOCK))), dim3(BLOCK), 0, c->stream,
                           c->tile_len, (unsigned long long)c->n_tiles, &c->scratch64[0]);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(&c->st->live_slots, &c->scratch64[0], 8, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

void free_corpus(yabpe_ctx *c) {
    dfree(c->tiles); dfree(c->tiles_alt); dfree(c->tile_len); dfree(c->tile_len_alt);
    dfree(c->tile_wbase); dfree(c->tile_wbase_alt); dfree(c->wfreq); dfree(c->sig);
    c->sig = nullptr; c->sig_stride = 0;
    dfree(c->long_tok); dfree(c->long_off); dfree(c->long_len); dfree(c->long_freq); dfree(c->long_sig);
    c->long_sig = nullptr; c->long_sig_stride = 0;
    c->tiles = c->tiles_alt = nullptr;
    c->tile_len = c->tile_len_alt = c->tile_wbase = c->tile_wbase_alt = c->wfreq = nullptr;
    c->long_tok = nullptr; c->long_off = nullptr; c->long_len = c->long_freq = nullptr;
    c->n_long = 0; c->n_tiles = 0;
    table_free(c->table);
    c->have_words = false;
}

void free_records(yabpe_ctx *c) {
    dfree(c->rec_left); dfree(c->rec_right); dfree(c->rec_merged);
    dfree(c->rec_count); dfree(c->rec_sites); dfree(c->rec_live);
    c->rec_left = c->rec_right = c->rec_merged = nullptr;
    c->rec_count = c->rec_sites = c->rec_live = nullptr;
    c->rec_cap = 0;
}


// (Re)compute every tile's signature from the resident stream (after load and after a retile).
int build_signatures(yabpe_ctx *c) {
    if (!optv(c, "skip_index", 1) || c->n_tiles == 0) return 0;
    if (!c->sig || c->sig_stride < c->n_tiles) {
        dfree(c->sig);
        c->sig = nullptr;
        c->sig_stride = (uint32_t)((c->n_tiles + 31u) & ~31u);  // rows start 128-B aligned
        TRY(dmalloc(c, &c->sig, (uint64_t)SIG_ROWS * c->sig_stride));
    }
    SigParams P{c->tiles, c->tile_len, c->n_tiles, c->sig, c->sig_stride};
    const uint32_t n_groups = (uint32_t)((c->n_tiles + SIG_TILES - 1) / SIG_TILES);
    hipLaunchKernelGGL(k_build_sig, dim3(std::min<uint32_t>(n_groups, 256 * 3)), dim3(BLOCK), 0, c->stream, P);
    c->sig_tokens_at_build = c->st_host->tokens_now;
    c->sig_builds++;
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Repack the live words of the flat layout into fresh, densely filled tiles (drops dead/empty words and PAD).
// The apply kernel reads tile prefixes only, so this is what keeps its traffic proportional to live tokens.
int retile_flat(yabpe_ctx *c) {
    if (c->n_tiles == 0) return 0;
    uint32_t *kept = nullptr;
    unsigned long long *base = nullptr;
    TRY(dmalloc(c, &kept, c->n_tiles));
    TRY(dmalloc(c, &base, (uint64_t)c->n_tiles + 1));
    const uint32_t grid = count_grid(c);
    RetileParams P{c->tiles, c->tile_len, c->n_tiles, kept, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_retile<false>, dim3(grid), dim3(BLOCK), 0, c->stream, P);
    HIPCHK(c, hipGetLastError());
    if (exclusive_scan<uint32_t>(c->stream, kept, c->n_tiles, base, (unsigned long long)c->n_tiles + 1) != 0)
        return fail(c, YABPE_E_HIP, "retile scan failed: %s", hipGetErrorString(hipGetLastError()));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, base + c->n_tiles, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t new_n = std::max<uint32_t>(1, (uint32_t)((total + SPAN - 1) / SPAN));
    if (!c->tiles_alt || c->tiles_alt_cap < new_n) {
        dfree(c->tiles_alt);
        dfree(c->tile_len_alt);
        c->tiles_alt = nullptr;
        c->tile_len_alt = nullptr;
        TRY(dmalloc(c, &c->tiles_alt, (uint64_t)new_n * CAP));
        TRY(dmalloc(c, &c->tile_len_alt, new_n));
        c->tiles_alt_cap = new_n;
    }
    // retile_form 1: new tiles gathered whole (k_retile_gather); 0: fill, then scatter element by element
    const bool gather = optv(c, "retile_form", 1) != 0;
    if (gather) {
        RetileGatherParams G{c->tiles, c->tile_len, c->n_tiles, base, c->tiles_alt, c->tile_len_alt, new_n};
        hipLaunchKernelGGL(k_retile_gather, dim3(cdiv64(new_n, RETILE_GROUP)), dim3(BLOCK), 0, c->stream, G);
    } else {
        TRY(fill_u16(c, c->tiles_alt, (uint64_t)new_n * CAP, YB_PAD));
        HIPCHK(c, hipMemsetAsync(c->tile_len_alt, 0, (size_t)new_n * 4, c->stream));
        P.base = base;
        P.new_tiles = c->tiles_alt;
        P.new_len = c->tile_len_alt;
        hipLaunchKernelGGL(k_retile<true>, dim3(grid), dim3(BLOCK), 0, c->stream, P);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(c->tiles, c->tiles_alt);
    std::swap(c->tile_len, c->tile_len_alt);
    std::swap(c->tiles_cap, c->tiles_alt_cap);
    c->n_tiles = new_n;
    dfree(kept);
    dfree(base);
    TRY(refresh_live_slots(c));
    if (c->sig_valid) TRY(build_signatures(c));
    c->stats.retiles++;
    return 0;
}

}  // namespace

namespace {
// *dst = src if it already is device memory with the asked alignment, else a copy of it that S owns (bytes == 0: src).
template <class T>
int to_device(yabpe_ctx *c, Scratch &S, const T *src, uint64_t bytes, uintptr_t align, const T **dst) {
    *dst = src;
    const bool on_dev = is_device_ptr(src);
    if (bytes == 0 || (on_dev && ((uintptr_t)src & (align - 1)) == 0)) return 0;
    uint8_t *own = nullptr;
    HIPCHK(c, S.get(&own, bytes));
    HIPCHK(c, hipMemcpy(own, src, bytes, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    *dst = (const T *)own;
    return 0;
}

// the document starts of encode (what = "text") and decode ("ids"): host array, validated before a kernel indexes with it
int check_starts(yabpe_ctx *c, const uint64_t *starts, uint32_t n, uint64_t limit, const char *what) {
    if (!starts || !n || starts[0] != 0) return fail(c, YABPE_E_INVALID, "doc_off must hold n_docs >= 1 starts, the first one 0");
    for (uint32_t d = 1; d < n; ++d)
        if (starts[d] < starts[d - 1] || starts[d] > limit) return fail(c, YABPE_E_INVALID, "document starts must ascend inside the %s", what);
    return 0;
}

// the chunk starts of the pre-tokeniser (what = "chunk") and the part starts of the text passes ("part"): *v = the host
// table, validated before a kernel indexes with it, or {0} when none is given
int offset_table(yabpe_ctx *c, const uint64_t *off, uint32_t n, uint64_t n_bytes, const char *what, std::vector<unsigned long long> *v) {
    v->clear();
    if (!off || !n) {
        v->push_back(0);
        return 0;
    }
    for (uint32_t k = 0; k < n; ++k) {
        if (off[k] > n_bytes || (k && off[k] < off[k - 1])) return fail(c, YABPE_E_INVALID, "%s offsets must ascend inside the text", what);
        v->push_back(off[k]);
    }
    if ((*v)[0] != 0) return fail(c, YABPE_E_INVALID, "the first %s must start at 0", what);
    return 0;
}

// the results a driver handed out and the context owns until that driver's next call or its *_free
void free_bufs(std::vector<void *> &bufs) {
    for (void *p : bufs) dfree(p);
    bufs.clear();
}

// ms[k] = ev[k] .. ev[k + 1] for every k < last (the rest stays as it is); -> ev[0] .. ev[last]
float pass_times(const hipEvent_t *ev, int last, float *ms) {
    float total = 0;
    for (int k = 0; k < last; ++k) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    (void)hipEventElapsedTime(&total, ev[0], ev[last]);
    return total;
}

// The front and the hand-out of the text-to-text passes (yabpe_normalize, yabpe_utf8_repair, yabpe_lowercase).  A pass runs
// its own argument checks, check(), builds its device tables, begin(), its kernels, and ends with hand_out_input() (the
// text needs no change, or is empty) or hand_out().  A call that check() refuses has freed nothing.
struct TextPass {
    yabpe_ctx *c;
    std::vector<void *> &bufs;  // the pass's results in the context: those of the last call go in begin(), the new ones are pushed here
    const uint8_t **out_text;
    uint64_t **out_off;
    uint64_t *out_n, *stat_n_out = nullptr;  // (the stats' n_bytes_out)
    Scratch S;
    std::vector<unsigned long long> parts;  // the part starts and the end: the offsets of an unchanged text
    const uint8_t *text = nullptr, *d_text = nullptr;
    unsigned long long n = 0, *d_parts = nullptr;
    uint32_t np = 0;

    TextPass(yabpe_ctx *c_, std::vector<void *> &bufs_, const uint8_t **out_text_, uint64_t **out_off_, uint64_t *out_n_)
        : c(c_), bufs(bufs_), out_text(out_text_), out_off(out_off_), out_n(out_n_), S(c_->device, c_->rank) {
        *out_text = nullptr; *out_off = nullptr; *out_n = 0;
    }
    int check(const uint8_t *text_, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts) {
        if (n_bytes && !text_) return fail(c, YABPE_E_INVALID, "text is NULL");
        TRY(offset_table(c, part_off, n_parts, n_bytes, "part", &parts));
        text = text_;
        n = n_bytes;
        np = (uint32_t)parts.size();
        parts.push_back(n_bytes);
        return 0;
    }
    // the last call's results freed, the stats reset, the events there; the text (at `align`) and the part table on the device
    template <class Stats, int NE>
    int begin(Stats &stats, hipEvent_t (&ev)[NE], uintptr_t align) {
        free_bufs(bufs);
        stats = Stats{};
        stats.n_bytes_in = n;
        stats.n_parts = np;
        stat_n_out = &stats.n_bytes_out;
        for (auto &e : ev)
            if (!e) HIPCHK(c, hipEventCreate(&e));
        TRY(to_device(c, S, text, n, align, &d_text));
        HIPCHK(c, S.get(&d_parts, parts.size()));
        HIPCHK(c, hipMemcpyAsync(d_parts, parts.data(), parts.size() * 8, hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    // the new text with its offsets (lowercase's same-size path: the input's, d_parts)
    int hand_out(uint8_t *out, unsigned long long *off, unsigned long long n_out) {
        bufs.push_back(S.take(out));
        return hand_out_as(out, off, n_out);
    }
    // the input and its offsets: the result when nothing changes, and of an empty text (then only the table upload is in flight)
    int hand_out_input() {
        if (n == 0) HIPCHK(c, hipStreamSynchronize(c->stream));
        if (d_text != text && n) bufs.push_back(S.take(const_cast<uint8_t *>(d_text)));  // (the staged text is handed out)
        return hand_out_as(n ? d_text : nullptr, d_parts, n);
    }
    int hand_out_as(const uint8_t *out, unsigned long long *off, unsigned long long n_out) {
        bufs.push_back(S.take(off));
        *out_text = out;
        *out_off = (uint64_t *)off;
        *out_n = *stat_n_out = n_out;
        return YABPE_OK;
    }
};

// ---- fixed-shape batches (yabpe_layout_pad / _pack / _windows / _pairs / _fit)
// flags outside mode_flags, the ones the call takes (an unknown flag is one of them)
int layout_flags(yabpe_ctx *c, const yabpe_layout_t *lay, uint32_t mode_flags) {
    if (lay->flags & ~mode_flags)
        return fail(c, YABPE_E_INVALID, "layout flags 0x%x do not belong to this call (it takes 0x%x)", lay->flags & ~mode_flags, mode_flags);
    return 0;
}

// What the layout calls share, as steps a call runs in order (between them: its own checks, buffers and kernels):
// begin(), count_begin(), [row_offsets(), row_budget(), write()], end().  lay_ev[0..1] bracket the lengths pass (windows and
// pairs: count + scan + rows), [2..3] the write kernel.  A call that its own checks or begin()'s refuse has freed nothing.
struct LayoutCall {
    yabpe_ctx *c;
    Scratch S;
    hipStream_t s;
    const yabpe_layout_t *lay = nullptr;
    const uint32_t *d_ids = nullptr;
    const unsigned long long *d_docs = nullptr;
    const ulonglong2 *d_spans = nullptr;            // NULL: the call stores no spans
    unsigned long long *counters = nullptr;         // 4 on the device; h_cnt: their values once row_offsets() has run
    unsigned long long h_cnt[4] = {0, 0, 0, 0};

    explicit LayoutCall(yabpe_ctx *c_) : c(c_), S(c_->device, c_->rank), s(c_->stream) {}
    LayConst K() const { return LayConst{lay->pad_id, lay->bos_id, lay->eos_id}; }

    // The arguments checked (mode_flags: the flags the call takes), the last layout released, the stats reset; the ids, the
    // validated document starts and the spans (if any) on the device, the counters allocated.
    int begin(const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t *n_docs, const uint64_t *spans, const yabpe_layout_t *lay_,
              uint32_t mode_flags) {
        if (!lay_) return fail(c, YABPE_E_INVALID, "layout is NULL");
        if (lay_->flags & ~(LAY_PAD_FLAGS | LAY_PACK_FLAGS)) return fail(c, YABPE_E_INVALID, "unknown layout flags 0x%x", lay_->flags);
        TRY(layout_flags(c, lay_, mode_flags));
        if (n_ids && !ids) return fail(c, YABPE_E_INVALID, "ids is NULL");
        if (!doc_off && *n_docs > 1) return fail(c, YABPE_E_INVALID, "doc_off is NULL with %u documents", *n_docs);
        // the document starts on the host (validated: the kernels index the ids with them) and on the device
        const bool docs_dev = doc_off && is_device_ptr(doc_off);
        if (!doc_off) *n_docs = 1;
        std::vector<uint64_t> h_docs(*n_docs, 0);
        if (doc_off && *n_docs) {
            if (docs_dev) HIPCHK(c, hipMemcpy(h_docs.data(), doc_off, (size_t)*n_docs * 8, hipMemcpyDeviceToHost));
            else memcpy(h_docs.data(), doc_off, (size_t)*n_docs * 8);
        }
        TRY(check_starts(c, h_docs.data(), *n_docs, n_ids, "ids"));
        yabpe_layout_free(c);
        c->lay_stats = yabpe_layout_stats_t{};
        c->lay_stats.n_ids = n_ids;
        c->lay_stats.n_docs = *n_docs;
        lay = lay_;
        for (auto &e : c->lay_ev)
            if (!e) HIPCHK(c, hipEventCreate(&e));
        TRY(to_device(c, S, ids, n_ids * 4, 4, &d_ids));
        TRY(to_device(c, S, docs_dev ? (const unsigned long long *)doc_off : (const unsigned long long *)h_docs.data(), (uint64_t)*n_docs * 8, 8, &d_docs));
        if (spans) TRY(to_device(c, S, (const ulonglong2 *)spans, n_ids * 16, 16, &d_spans));
        HIPCHK(c, S.get(&counters, 4));
        return 0;
    }
    // the lengths pass starts: its event, the counters zeroed (the call's own buffers are allocated before, outside the bracket)
    int count_begin() {
        HIPCHK(c, hipEventRecord(c->lay_ev[0], s));
        HIPCHK(c, hipMemsetAsync(counters, 0, 32, s));
        return 0;
    }
    // Row offsets: the exclusive scan of cnt[n] into row_off[n + 1] and its total -> *n_rows (cnt NULL: one row each, *n_rows
    // stays as it is); the counters -> h_cnt.  The stream is idle afterwards.
    int row_offsets(const unsigned long long *cnt, uint32_t n, unsigned long long *row_off, unsigned long long *n_rows) {
        if (cnt) {
            if (exclusive_scan<unsigned long long>(s, cnt, n, row_off, (unsigned long long)n + 1) != 0)
                return fail(c, YABPE_E_HIP, "scan of the row counts failed");
            HIPCHK(c, hipMemcpyAsync(n_rows, row_off + n, 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipMemcpyAsync(h_cnt, counters, 32, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return 0;
    }
    // Row budget: the longest document (h_cnt[0]) fits the u32 per-row arrays (`u32_fields` names them), n_rows rows fit one call
    int row_budget(const char *u32_fields, unsigned long long n_rows, unsigned long long *n_slots) {
        if (h_cnt[0] > 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a document of %llu ids: %s u32", h_cnt[0], u32_fields);
        if (n_rows > LAY_MAX_SLOTS / lay->row_len)
            return fail(c, YABPE_E_CAPACITY, "%llu rows of %u slots: at most 2^36 slots in one call", n_rows, lay->row_len);
        *n_slots = n_rows * lay->row_len;
        return 0;
    }
    // The lengths pass ends behind the rows kernel; the record-driven write of windows and pairs into the slots of lay_buf
    // (n_slots >= 1: a document has at least one row).
    template <class Row>
    int write(const Row &R, const typename Row::Rec *rec, unsigned long long n_rows, unsigned long long n_slots) {
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->lay_ev[1], s));
        HIPCHK(c, hipEventRecord(c->lay_ev[2], s));
        const LayRowsParams<Row> W{d_ids, rec, n_rows, lay->row_len, lay->flags, R, K(), c->lay_buf[LB_ROWS], (uint8_t *)c->lay_buf[LB_TYPES], n_slots,
                                   d_spans, (ulonglong2 *)c->lay_buf[LB_SPANS]};
        if (d_spans)
            hipLaunchKernelGGL((k_lay_rows_write<Row, true>), dim3(cdiv64(n_slots, LAY_PIECE)), dim3(BLOCK), 0, s, W);
        else
            hipLaunchKernelGGL((k_lay_rows_write<Row, false>), dim3(cdiv64(n_slots, LAY_PIECE)), dim3(BLOCK), 0, s, W);
        return 0;
    }
    // the write pass ends: every call's success path synchronises here; the times of the passes
    int end() {
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->lay_ev[3], s));
        const hipError_t se = hipStreamSynchronize(s);
        if (se != hipSuccess) {
            yabpe_layout_free(c);
            return fail(c, YABPE_E_HIP, "layout kernels failed: %s", hipGetErrorString(se));
        }
        float ms[3] = {0, 0, 0};
        c->lay_stats.total_ms = pass_times(c->lay_ev, 3, ms);
        c->lay_stats.lengths_ms = ms[0];
        c->lay_stats.write_ms = ms[2];
        return 0;
    }
    // ... and the stats of a call whose count kernel sums the counters (pad, windows, pairs)
    int end(unsigned long long n_rows, unsigned long long row_len, unsigned long long n_slots) {
        TRY(end());
        auto &st = c->lay_stats;
        st.n_rows = n_rows;
        st.row_len = row_len;
        st.n_truncated_docs = h_cnt[1];
        st.n_ids_dropped = h_cnt[2];
        st.n_pad_slots = n_slots - h_cnt[3];
        return 0;
    }
};

// The documents stably by their keys (fit_logic.h), in `passes` radix passes of 8 bits from the lowest digit; *sorted = the
// documents in that order (a buffer of S).
int fit_sort(yabpe_ctx *c, Scratch &S, hipStream_t s, const uint32_t *key, uint32_t n, uint32_t passes, const uint32_t **sorted) {
    const uint32_t n_tiles = cdiv64(n, FIT_SORT_TILE);
    const unsigned long long n_counts = (unsigned long long)BLOCK * n_tiles;
    uint32_t *kbuf[2] = {nullptr, nullptr}, *vbuf[2] = {nullptr, nullptr}, *counts = nullptr;
    unsigned long long *offs = nullptr;
    for (int k = 0; k < 2; ++k) {
        HIPCHK(c, S.get(&kbuf[k], n));
        HIPCHK(c, S.get(&vbuf[k], n));
    }
    HIPCHK(c, S.get(&counts, n_counts));
    HIPCHK(c, S.get(&offs, n_counts));
    const uint32_t *kin = key, *vin = nullptr;  // (the first pass reads the identity)
    for (uint32_t pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(k_fit_sort_count, dim3(n_tiles), dim3(BLOCK), 0, s, kin, n, pass, counts, n_tiles);
        HIPCHK(c, hipGetLastError());
        if (exclusive_scan<uint32_t>(s, counts, n_counts, offs, n_counts) != 0) return fail(c, YABPE_E_HIP, "scan of the digit counts failed");
        hipLaunchKernelGGL(k_fit_sort_scatter, dim3(n_tiles), dim3(BLOCK), 0, s,
                           FitScatterParams{kin, vin, n, pass, offs, n_tiles, kbuf[pass & 1], vbuf[pass & 1]});
        HIPCHK(c, hipGetLastError());
        kin = kbuf[pass & 1];
        vin = vbuf[pass & 1];
    }
    *sorted = vin;
    return 0;
}

// ---- what the u16 and the u32 drivers share (yabpe_id32_host.h): the differences between the two stay with the callers
// N timing events of one call: destroyed on every way out
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    hipError_t create() {
        for (hipEvent_t &x : e) {
            const hipError_t r = hipEventCreate(&x);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// The base vocabulary on the host: every token's bytes at a multiple of 4 in the pool (new tokens' bytes are written four
// at a time); order[r] = the id of byte-order rank r; one TokRec per id with rank 0.
struct BaseVocab {
    std::vector<uint32_t> off, len, order;
    std::vector<uint8_t> pool;
    std::vector<TokRec> rec;
};
void base_vocab_pack(const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tokens, BaseVocab &V) {
    V.off.resize(n_tokens); V.len.resize(n_tokens); V.order.resize(n_tokens);
    for (uint32_t i = 0; i < n_tokens; ++i) {
        V.len[i] = tok_off[i + 1] - tok_off[i];
        V.off[i] = (uint32_t)V.pool.size();
        V.pool.insert(V.pool.end(), tok_bytes + tok_off[i], tok_bytes + tok_off[i + 1]);
        V.pool.resize((V.pool.size() + 3) & ~(size_t)3, 0);
        V.order[i] = i;
    }
}
int base_vocab_index(yabpe_ctx *c, BaseVocab &V) {
    const uint32_t n_tokens = (uint32_t)V.len.size();
    auto cmp = [&](uint32_t x, uint32_t y) {
        uint32_t n = std::min(V.len[x], V.len[y]);
        int d = memcmp(V.pool.data() + V.off[x], V.pool.data() + V.off[y], n);
        if (d) return d < 0;
        return V.len[x] < V.len[y];
    };
    std::sort(V.order.begin(), V.order.end(), cmp);
    for (uint32_t r = 1; r < n_tokens; ++r)
        if (!cmp(V.order[r - 1], V.order[r])) return fail(c, YABPE_E_INVALID, "duplicate token bytes in the base vocabulary (trainer.py:130)");
    V.rec.resize(n_tokens);
    for (uint32_t i = 0; i < n_tokens; ++i) {
        V.rec[i].rank = 0;
        V.rec[i].len = V.len[i];
        V.rec[i].hash = yb_hash_bytes(V.pool.data() + V.off[i], V.len[i]);
        V.rec[i].pre8 = yb_pre8(V.pool.data() + V.off[i], V.len[i]);
        V.rec[i].pad = 0;
    }
    return 0;
}
// the byte-string set of tokens [0, n_tokens) in a fresh array of vset_cap slots
int upload_vset(yabpe_ctx *c, const std::vector<TokRec> &rec, uint32_t n_tokens, uint32_t vset_cap) {
    std::vector<unsigned long long> vset(vset_cap, VSET_EMPTY);
    const uint32_t mask = vset_cap - 1;
    for (uint32_t i = 0; i < n_tokens; ++i) {
        uint32_t s = yb_vset_home(rec[i].hash, rec[i].len) & mask;
        while (vset[s] != VSET_EMPTY) s = (s + 1) & mask;
        vset[s] = yb_vset_entry(i, rec[i].hash);
    }
    dfree(c->tt.vset);
    c->tt.vset = nullptr;
    TRY(dmalloc(c, &c->tt.vset, vset_cap));
    HIPCHK(c, hipMemcpy(c->tt.vset, vset.data(), (size_t)vset_cap * 8, hipMemcpyHostToDevice));
    c->tt.vset_mask = mask;
    return 0;
}
// the token table on the device at the capacities the caller chose, and a state that knows nothing but these tokens
int base_vocab_upload(yabpe_ctx *c, const BaseVocab &V, uint32_t pool_cap, uint32_t tok_cap, uint32_t vset_cap) {
    const uint32_t n_tokens = (uint32_t)V.len.size();
    dfree(c->tt.pool); dfree(c->tt.off); dfree(c->tt.len); dfree(c->tt.rec);
    c->tt.pool = nullptr; c->tt.off = c->tt.len = nullptr; c->tt.rec = nullptr;
    TRY(dmalloc(c, &c->tt.pool, pool_cap));
    TRY(dmalloc(c, &c->tt.off, tok_cap));
    TRY(dmalloc(c, &c->tt.len, tok_cap));
    TRY(dmalloc(c, &c->tt.rec, tok_cap));
    c->tt.pool_cap = pool_cap;
    TRY(upload_vset(c, V.rec, n_tokens, vset_cap));
    HIPCHK(c, hipMemset(c->tt.pool, 0, pool_cap));
    HIPCHK(c, hipMemcpy(c->tt.pool, V.pool.data(), V.pool.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->tt.off, V.off.data(), (size_t)n_tokens * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->tt.len, V.len.data(), (size_t)n_tokens * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->tt.rec, V.rec.data(), (size_t)n_tokens * sizeof(TokRec), hipMemcpyHostToDevice));
    TRY(state_pull(c));
    DevState *h = c->st_host;
    memset(h, 0, sizeof(DevState));
    h->n_tokens = n_tokens;
    h->pool_used = (uint32_t)V.pool.size();
    TRY(state_push(c));
    c->base_tokens = n_tokens;
    c->have_vocab = true;
    c->id_bits_fixed = true;
    return YABPE_OK;
}

// A load's arguments, checked before anything of the loaded corpus is given up.  *max_token_bytes: DESIGN.md (m), a property
// of the load -- read here, fixed until the next load.
int load_check_args(yabpe_ctx *c, const uint64_t *word_off, uint64_t n_words, int64_t *max_token_bytes) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_vocab) return fail(c, YABPE_E_INVALID, "call yabpe_set_vocab first");
    if (!word_off) return fail(c, YABPE_E_INVALID, "word_off is NULL");
    if (n_words >= 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "more than 2^32-2 words per context");
    *max_token_bytes = optv(c, "max_token_bytes", 0);
    if (!yb_limit_valid(*max_token_bytes))
        return fail(c, YABPE_E_INVALID, "max_token_bytes is %lld: 0 (no limit) or a length of at least %u bytes", (long long)*max_token_bytes, YB_LIMIT_MIN);
    return 0;
}
// The words of a load on the device (offsets stay absolute: `bytes` is biased by -off_base), equal words pooled if asked
// (trainer.py:221-225).  The staged copies belong to `In`, the pooled words to `S`: a caller that needs nothing else of
// `In` releases it when `pooled` comes back set.  ev0 is recorded between the staging and the pooling.
struct LoadInputs {
    const unsigned long long *off = nullptr, *freq = nullptr;
    const uint8_t *bytes = nullptr;
    uint64_t n_words = 0, total_bytes = 0, off_base = 0;
    bool pooled = false;
};
int load_stage_inputs(yabpe_ctx *c, Scratch &In, Scratch &S, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq,
                      uint64_t n_words, uint32_t flags, hipEvent_t ev0, LoadInputs *L) {
    L->bytes = bytes;
    L->n_words = n_words;
    if (is_device_ptr(word_off)) {
        HIPCHK(c, hipMemcpy(&L->total_bytes, word_off + n_words, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&L->off_base, word_off, 8, hipMemcpyDeviceToHost));
        L->total_bytes -= L->off_base;
    } else {
        L->off_base = word_off[0];
        L->total_bytes = word_off[n_words] - L->off_base;
    }
    TRY(to_device(c, In, (const unsigned long long *)word_off, (n_words + 1) * 8, 1, &L->off));
    if (L->total_bytes && !bytes) return fail(c, YABPE_E_INVALID, "bytes is NULL");
    if (L->total_bytes) {
        TRY(to_device(c, In, bytes + L->off_base, L->total_bytes, 1, &L->bytes));
        L->bytes -= L->off_base;
    }
    if (word_freq) TRY(to_device(c, In, (const unsigned long long *)word_freq, n_words * 8, 1, &L->freq));
    HIPCHK(c, hipEventRecord(ev0, c->stream));
    c->n_words_input = n_words;
    if ((flags & YABPE_LOAD_DEDUP) && n_words > 0) {
        DedupOut dd{};
        int r = dedup_words(c->stream, L->bytes, L->off, L->freq, n_words, &dd);
        if (r != 0) return fail(c, YABPE_E_HIP, "device dedup failed (%d): %s", r, hipGetErrorString(hipGetLastError()));
        S.adopt(dd.bytes); S.adopt(dd.off); S.adopt(dd.freq);
        L->bytes = dd.bytes; L->off = dd.off; L->freq = dd.freq;
        L->n_words = dd.n_unique;
        L->total_bytes = dd.total_bytes;
        L->off_base = 0;
        L->pooled = true;
    }
    return 0;
}

// ---- the load driver (DESIGN.md "Host drivers"): one run state, and the steps that both id widths run.  The u16 load's own
// steps stand in front of load_words_impl, the u32 load's in yabpe_id32_host.h.
struct LoadRun {
    yabpe_ctx *c;
    Scratch In, S;  // the staged inputs; every other temporary of the load: pooled words, walk buffers, long-word lists
    Events<3> ev;  // start, end, words replayed
    LoadInputs L;
    int64_t max_token_bytes = 0;
    uint64_t total_tokens = 0;  // tokens of the words: their bytes, or what the replay leaves of them
    const RpTable *rp = nullptr;             // the u16 resumed load: the model's table, and what the replay wrote:
    uint32_t *d_wcnt = nullptr;              // tokens per word after the replay ...
    uint16_t *d_wtok = nullptr;              // ... the tokens, word w's where its bytes start ...
    unsigned long long *d_tokoff = nullptr;  // ... and the exclusive scan of the counts
    uint32_t *d_long_word = nullptr;         // the u16 load: the words that go to the long-word buffers
    explicit LoadRun(yabpe_ctx *c_) : c(c_), In(c_->device, c_->rank), S(c_->device, c_->rank) {}
};

// The loaded corpus given up, the new words on the device, the context told how many (a rank without words still runs the
// layout of its peers: the collectives differ).  early_release: the staged inputs go as soon as pooled words replace them.
int load_begin(LoadRun &R, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words, uint32_t flags, bool early_release) {
    yabpe_ctx *c = R.c;
    free_corpus(c);
    HIPCHK(c, R.ev.create());
    TRY(load_stage_inputs(c, R.In, R.S, bytes, word_off, word_freq, n_words, flags, R.ev.e[0], &R.L));
    if (early_release && R.L.pooled) R.In.release();
    c->weighted = R.L.freq != nullptr || (flags & YABPE_LOAD_DEDUP) != 0;
    c->n_words = R.L.n_words;
    c->tokens_initial = R.total_tokens = R.L.total_bytes;
    return 0;
}

// The device state of a fresh job (trainer.py:227-235: the pair count follows; tok_len is in place before the first key enters
// the table, so that count leaves out what is too long).  live_slots: known already, they travel with this push; NULL: counted later.
int load_state_reset(yabpe_ctx *c, uint64_t total_tokens, int64_t max_token_bytes, const unsigned long long *live_slots = nullptr) {
    TRY(state_pull(c));
    DevState *h = c->st_host;
    h->iter = 0; h->done = 0; h->halt = 0; h->halt_req = 0; h->sites = 0;
    h->tokens_now = total_tokens;
    h->table_entries = 0;
    if (live_slots) h->live_slots = *live_slots;
    h->tok_len = c->tt.len;
    h->max_token_bytes = (uint32_t)max_token_bytes;
    return state_push(c);
}

// Everything that starts over with a new corpus.  The whole statistics struct: every field of yabpe_stats_t is either a sum
// that the calls after a load add to (the times, launches, merges and bytes of the phases, retiles, table_rebuilds -- the
// load's own rebuild is not counted) or is assigned by yabpe_stats() on every call from the context and the device state
// (n_words .. table_entries, scan_skip_*, cand_*, fused_launches, exchange*, pool_growths); load_ms is stored by the caller
// after this.  Then the context's counters behind those fields, and the exchange's adaptive size.
int job_reset(yabpe_ctx *c) {
    c->stats = yabpe_stats_t{};
    c->scan_skip_launches = c->cand_rebuilds = c->cand_rescans = c->fused_launches = c->exchanges = 0;
    c->cand_margin = CAND_MARGIN_FIRST;  // (as a fresh context: what the last job's counts made of it says nothing about this one's)
    c->xeff = c->xcap;  // (a new job starts with whole buffers: its first merges are its densest)
    c->xseen[0] = c->xseen[1] = c->xseen[2] = c->xseen[3] = 0;
    c->xeff_sum = c->exchange_growths = c->exchange_max_records = 0;
    if (c->blk_read) HIPCHK(c, hipMemsetAsync(c->blk_read, 0, 2 * MAX_LISTS * 8, c->stream));  // (the statistics; the counter word keeps its tag)
    return 0;
}

// The end of a load: the clock read, a new job's counters, the words declared loaded.  replayed: the load recorded ev.e[2]
// when its words were replayed -- what came before and after it goes to resume_stats, with the long words.
int load_account(LoadRun &R, bool replayed) {
    yabpe_ctx *c = R.c;
    HIPCHK(c, hipEventRecord(R.ev.e[1], c->stream));
    HIPCHK(c, hipEventSynchronize(R.ev.e[1]));
    float ms = 0, sms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, R.ev.e[0], R.ev.e[1]));
    if (replayed) {
        HIPCHK(c, hipEventElapsedTime(&sms, R.ev.e[0], R.ev.e[2]));
        c->resume_stats.segment_ms = sms;  // (pooling of equal words included)
        c->resume_stats.build_ms = ms - sms;
        c->resume_stats.n_long = c->n_long;
    }
    TRY(job_reset(c));
    c->stats.load_ms = ms;
    c->have_words = true;
    return YABPE_OK;
}

// The merge triples of a resumed load against the vocabulary: every id exists, every merged token is as long as its operands.
int check_merge_triples(yabpe_ctx *c, const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges) {
    TRY(state_pull(c));
    const uint32_t n_tokens = c->st_host->n_tokens;
    std::vector<uint32_t> len(n_tokens);
    HIPCHK(c, hipMemcpy(len.data(), c->tt.len, (size_t)n_tokens * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_merges; ++i) {
        const uint32_t l = left[i], r = right[i], m = merged[i];
        if (l >= n_tokens || r >= n_tokens || m >= n_tokens)
            return fail(c, YABPE_E_INVALID, "merge %u names token id %u, the vocabulary has %u", i, std::max(l, std::max(r, m)), n_tokens);
        if (len[m] != len[l] + len[r])
            return fail(c, YABPE_E_INVALID, "merge %u: token %u has %u bytes, its operands %u + %u", i, m, len[m], len[l], len[r]);
    }
    return 0;
}

// The replay table of either width (rp_build_table) in device memory that S owns.
template <class W>
int rp_upload(yabpe_ctx *c, Scratch &S, const RpTableHostT<W> &th, RpTableT<W> *t) {
    t->mask = (uint32_t)th.idx_key.size() - 1u;
    TRY(to_device(c, S, th.idx_key.data(), th.idx_key.size() * sizeof(typename W::key_t), 1, &t->idx_key));
    TRY(to_device(c, S, th.idx_first.data(), th.idx_first.size() * 4, 1, &t->idx_first));
    return to_device(c, S, th.ent.data(), th.ent.size() * sizeof(RpEntryT<W>), 1, &t->ent);
}

// ---- the u16 load's own steps over one LoadRun (the steps both widths run: load_begin .. load_account)
// Resumed load: every word rewritten by the model's merges (replay_logic.h); the tiles step places it by its token count.
int load_replay(LoadRun &R) {
    yabpe_ctx *c = R.c;
    const LoadInputs &L = R.L;
    const uint64_t n_words = L.n_words;
    c->resume_stats = yabpe_resume_stats_t{};
    c->resume_stats.n_unique = n_words;
    if (n_words) {
        Scratch &S = R.S;
        uint32_t *d_llen = nullptr, *d_ltok = nullptr, *d_lnxt = nullptr, *d_lprv = nullptr;
        unsigned long long *d_lbase = nullptr, *d_lheap = nullptr;
        HIPCHK(c, S.get(&R.d_wcnt, n_words)); HIPCHK(c, S.get(&R.d_wtok, L.total_bytes));
        HIPCHK(c, S.get(&R.d_tokoff, n_words + 1));
        HIPCHK(c, S.get(&d_llen, n_words)); HIPCHK(c, S.get(&d_lbase, n_words + 1));
        HIPCHK(c, hipMemsetAsync(&c->scratch64[2], 0, 8, c->stream));
        hipLaunchKernelGGL(k_replay_llen, dim3(cdiv64(n_words, 256)), dim3(256), 0, c->stream, L.off, (unsigned long long)n_words, d_llen, (uint32_t *)&c->scratch64[2]);
        HIPCHK(c, hipGetLastError());
        if (exclusive_scan<uint32_t>(c->stream, d_llen, n_words, d_lbase, (unsigned long long)n_words + 1) != 0)
            return fail(c, YABPE_E_HIP, "scan of the long words failed: %s", hipGetErrorString(hipGetLastError()));
        unsigned long long long_bytes = 0, too_long = 0;
        HIPCHK(c, hipMemcpyAsync(&long_bytes, d_lbase + n_words, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&too_long, &c->scratch64[2], 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (too_long & 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a single word longer than 2^32-1 bytes");
        if (long_bytes) {
            HIPCHK(c, S.get(&d_ltok, long_bytes)); HIPCHK(c, S.get(&d_lnxt, long_bytes));
            HIPCHK(c, S.get(&d_lprv, long_bytes)); HIPCHK(c, S.get(&d_lheap, 3 * long_bytes));
        }
        ReplayWordsParams RW{L.bytes, L.off, (unsigned long long)L.off_base, (unsigned long long)n_words, d_lbase, *R.rp, R.d_wcnt, R.d_wtok, d_ltok, d_lnxt, d_lprv, d_lheap};
        const uint32_t grid = (uint32_t)std::min<uint64_t>(cdiv64(n_words, WPB), (uint64_t)std::max(1, c->n_cu) * 8);
        hipLaunchKernelGGL(k_replay_words, dim3(grid), dim3(BLOCK), 0, c->stream, RW);
        HIPCHK(c, hipGetLastError());
        if (exclusive_scan<uint32_t>(c->stream, R.d_wcnt, n_words, R.d_tokoff, (unsigned long long)n_words + 1) != 0)
            return fail(c, YABPE_E_HIP, "scan of the token counts failed: %s", hipGetErrorString(hipGetLastError()));
        unsigned long long tt = 0;
        HIPCHK(c, hipMemcpyAsync(&tt, R.d_tokoff + n_words, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        R.total_tokens = tt;
        for (void *p : {(void *)d_llen, (void *)d_lbase, (void *)d_ltok, (void *)d_lnxt, (void *)d_lprv, (void *)d_lheap})
            S.release(p);  // (the walk buffers: gone before the tiles are allocated)
    }
    HIPCHK(c, hipEventRecord(R.ev.e[2], c->stream));
    c->tokens_initial = R.total_tokens;
    c->resume_stats.tokens = R.total_tokens;
    return 0;
}

// The one place that chooses among the three loaders: the replayed tokens (k_load_words_tok), or the bytes in load_form 1
// (k_load_tiles: every tile written whole) or 0 (k_load_words: one thread per word into tiles filled beforehand).
int load_launch_loader(LoadRun &R, bool tile_form, uint32_t long_cap) {
    yabpe_ctx *c = R.c;
    const LoadInputs &L = R.L;
    const LoadParams P{L.bytes, L.off, (unsigned long long)L.off_base, (unsigned long long)L.n_words, c->tiles, c->tile_len, c->tile_wbase,
                       (uint32_t *)&c->scratch64[2], &c->scratch64[3], R.d_long_word, long_cap};
    if (R.rp) {
        LoadTokParams Q{R.d_wtok, R.d_wcnt, R.d_tokoff, L.off, (unsigned long long)L.off_base, (unsigned long long)L.n_words, c->tiles, c->tile_len,
                        c->tile_wbase, P.long_count, P.long_total, R.d_long_word, long_cap};
        hipLaunchKernelGGL(k_load_words_tok, dim3(cdiv64(L.n_words, BLOCK)), dim3(BLOCK), 0, c->stream, Q);
    } else if (tile_form) {
        LoadTilesParams T{P, (unsigned long long)(L.off_base + L.total_bytes), c->n_tiles};
        hipLaunchKernelGGL(k_load_tiles, dim3(cdiv64(c->n_tiles, WPB * YB_LOAD_RUN)), dim3(BLOCK), 0, c->stream, T);
    } else {
        hipLaunchKernelGGL(k_load_words, dim3(cdiv64(L.n_words, BLOCK)), dim3(BLOCK), 0, c->stream, P);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The tiles sized and allocated, the words loaded into them: at most twice, the second time with a long-word list as long
// as the first attempt asked for.
int load_tiles(LoadRun &R) {
    yabpe_ctx *c = R.c;
    const uint64_t n_words = R.L.n_words;
    const uint64_t packed = R.total_tokens + n_words;
    const uint64_t n_tiles64 = (packed + SPAN - 1) / SPAN;
    if (n_tiles64 >= 0xFFFFFFF0ull) return fail(c, YABPE_E_CAPACITY, "corpus too large for one context");
    c->n_tiles = (uint32_t)n_tiles64;
    c->tiles_cap = c->n_tiles;
    c->tiles_alt_cap = 0;
    TRY(dmalloc(c, &c->tiles, (uint64_t)c->n_tiles * CAP));
    TRY(dmalloc(c, &c->tile_len, c->n_tiles));
    if (c->weighted) {
        TRY(dmalloc(c, &c->tile_wbase, c->n_tiles));
        TRY(dmalloc(c, &c->wfreq, n_words));
        HIPCHK(c, hipMemsetAsync(&c->scratch64[1], 0, 8, c->stream));
        if (n_words) {
            hipLaunchKernelGGL(k_freq64_to_32, dim3(cdiv64(n_words, 256)), dim3(256), 0, c->stream, R.L.freq, c->wfreq,
                               (unsigned long long)n_words, (uint32_t *)&c->scratch64[1]);
            HIPCHK(c, hipGetLastError());
        }
    }
    uint32_t long_cap = (uint32_t)optv(c, "long_cap", 1 << 16);
    // load_form 1: the byte paths write every tile whole (k_load_tiles), nothing to fill or clear first; 0: one thread per word
    const bool tile_form = !R.rp && optv(c, "load_form", 1) != 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!tile_form) {
            TRY(fill_u16(c, c->tiles, (uint64_t)c->n_tiles * CAP, YB_PAD));
            HIPCHK(c, hipMemsetAsync(c->tile_len, 0, (size_t)c->n_tiles * 4, c->stream));
            if (c->weighted) TRY(fill_u32(c, c->tile_wbase, c->n_tiles, 0xFFFFFFFFu));
        }
        HIPCHK(c, hipMemsetAsync(&c->scratch64[2], 0, 16, c->stream));  // [2] = long count (u32), [3] = long tokens
        R.S.release(R.d_long_word);
        HIPCHK(c, R.S.get(&R.d_long_word, long_cap));
        if (n_words) TRY(load_launch_loader(R, tile_form, long_cap));
        unsigned long long host2[2];
        HIPCHK(c, hipMemcpyAsync(host2, &c->scratch64[2], 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->n_long = (uint32_t)(host2[0] & 0xFFFFFFFFu);
        c->long_tokens = host2[1];
        if (c->n_long <= long_cap) break;
        long_cap = c->n_long;
        if (attempt == 1) return fail(c, YABPE_E_INTERNAL, "long-word list overflow");
    }
    if (c->weighted) {
        unsigned long long ov = 0;
        HIPCHK(c, hipMemcpy(&ov, &c->scratch64[1], 8, hipMemcpyDeviceToHost));
        if (ov & 0xFFFFFFFFu) return fail(c, YABPE_E_CAPACITY, "a word frequency exceeds 2^32-1");
    }
    // every word of the shard is a long one: the tiles counted for their bytes hold no word (a placeholder each in the weighted
    // layout, read by nobody without a word beside it) -- this rank keeps no tile and launches no apply kernel over them
    if (c->n_long && c->n_long == n_words) {
        dfree(c->tiles); dfree(c->tile_len); dfree(c->tile_wbase);
        c->tiles = nullptr; c->tile_len = c->tile_wbase = nullptr;
        c->n_tiles = c->tiles_cap = 0;
    }
    return 0;
}

// The long words: a buffer of their own, one workgroup per word.
int load_long_words(LoadRun &R) {
    yabpe_ctx *c = R.c;
    const LoadInputs &L = R.L;
    uint32_t *const d_long_word = R.d_long_word, *d_ll = nullptr;
    std::vector<uint32_t> lw(c->n_long);
    HIPCHK(c, hipMemcpy(lw.data(), d_long_word, (size_t)c->n_long * 4, hipMemcpyDeviceToHost));
    std::sort(lw.begin(), lw.end());  // deterministic layout
    HIPCHK(c, hipMemcpy(d_long_word, lw.data(), (size_t)c->n_long * 4, hipMemcpyHostToDevice));
    // where each long word goes: prefix sum of their lengths, on the device
    HIPCHK(c, R.S.get(&d_ll, c->n_long));
    TRY(dmalloc(c, &c->long_off, c->n_long + 1));
    HIPCHK(c, hipMemsetAsync(&c->scratch64[2], 0, 8, c->stream));
    if (R.rp)
        hipLaunchKernelGGL(k_long_lengths_tok, dim3(cdiv64(c->n_long, 256)), dim3(256), 0, c->stream, R.d_wcnt, d_long_word, c->n_long, d_ll);
    else
        hipLaunchKernelGGL(k_long_lengths, dim3(cdiv64(c->n_long, 256)), dim3(256), 0, c->stream, L.off, d_long_word, c->n_long, d_ll, (uint32_t *)&c->scratch64[2]);
    HIPCHK(c, hipGetLastError());
    if (exclusive_scan<uint32_t>(c->stream, d_ll, c->n_long, c->long_off, (unsigned long long)c->n_long + 1) != 0)
        return fail(c, YABPE_E_HIP, "long-word scan failed: %s", hipGetErrorString(hipGetLastError()));
    unsigned long long long_total = 0, too_long = 0;
    // (on the context's stream: it does not synchronise with the null stream, and a one-block scan returns without waiting)
    HIPCHK(c, hipMemcpyAsync(&long_total, c->long_off + c->n_long, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&too_long, &c->scratch64[2], 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    R.S.release(d_ll);
    if (too_long & 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a single word longer than 2^32-1 bytes");
    TRY(dmalloc(c, &c->long_tok, long_total));
    TRY(dmalloc(c, &c->long_len, c->n_long));
    if (c->weighted) TRY(dmalloc(c, &c->long_freq, c->n_long));
    if (R.rp) {
        LoadLongTokParams Q{R.d_wtok, R.d_wcnt, L.off, (unsigned long long)L.off_base, L.freq, d_long_word, c->long_off, c->long_tok, c->long_len, c->long_freq, c->n_long};
        hipLaunchKernelGGL(k_load_long_tok, dim3(c->n_long), dim3(BLOCK), 0, c->stream, Q);
    } else {
        LoadLongParams Q{L.bytes, L.off, L.freq, d_long_word, c->long_off, c->long_tok, c->long_len, c->long_freq, c->n_long};
        hipLaunchKernelGGL(k_load_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, Q);
    }
    HIPCHK(c, hipGetLastError());
    if (optv(c, "long_sig", 1)) {  // signatures: a merge whose pair is in no long word then costs 8 bytes per long word
        c->long_sig_stride = (c->n_long + 31u) & ~31u;
        TRY(dmalloc(c, &c->long_sig, (uint64_t)SIG_ROWS * c->long_sig_stride));
        LongParams G{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, PairTable{}, c->st, c->long_sig, c->long_sig_stride};
        hipLaunchKernelGGL(k_build_sig_long, dim3(c->n_long), dim3(BLOCK), 0, c->stream, G);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// The temporaries gone, the state of a fresh job, the initial pair count (trainer.py:227-235), the accounts.
int load_finish(LoadRun &R) {
    yabpe_ctx *c = R.c;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    R.In.release(); R.S.release();  // (before the pair table is built)
    TRY(load_state_reset(c, R.total_tokens, R.max_token_bytes));
    TRY(refresh_live_slots(c));
    c->sig_valid = false;
    // 65,536 possible byte pairs: start at load <= 1/4.  A resumed job's tokens are not bytes: the generic count, and a table
    // that grows until its load is <= 1/2 (table_rebuild)
    TRY(table_rebuild(c, 1ull << 18, /*all_bytes=*/R.rp == nullptr));
    return load_account(R, /*replayed=*/R.rp != nullptr);  // (a plain load leaves resume_stats as the last resumed load wrote it)
}

// rp != NULL: the words are brought to the state the model's merges leave them in before they are tiled (the table's
// arrays are device memory; pooled layout only)
int load_words_impl(yabpe_ctx *c, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words, uint32_t flags, const RpTable *rp) {
    LoadRun R(c);
    R.rp = rp;
    TRY(load_check_args(c, word_off, n_words, &R.max_token_bytes));
    TRY(load_begin(R, bytes, word_off, word_freq, n_words, flags, /*early_release=*/true));  // (the pooled words replace the staged inputs at once)
    if (rp) TRY(load_replay(R));
    TRY(load_tiles(R));
    if (c->n_long) TRY(load_long_words(R));
    return load_finish(R);
}

// Room for `need` per-merge records; the first `keep` entries survive a move.
int reserve_records(yabpe_ctx *c, uint32_t need, uint32_t keep) {
    if (c->rec_cap >= need) return 0;
    const uint32_t ncap = std::max<uint32_t>(need, c->rec_cap + c->rec_cap / 2);
    uint32_t *nl = nullptr, *nr = nullptr, *nm = nullptr;
    unsigned long long *nc = nullptr, *ns = nullptr, *nv = nullptr;
    TRY(dmalloc(c, &nl, ncap)); TRY(dmalloc(c, &nr, ncap)); TRY(dmalloc(c, &nm, ncap));
    TRY(dmalloc(c, &nc, ncap)); TRY(dmalloc(c, &ns, ncap)); TRY(dmalloc(c, &nv, ncap));
    HIPCHK(c, hipMemsetAsync(ns, 0, (size_t)ncap * 8, c->stream));
    if (c->rec_cap && keep) {
        const size_t n = keep;
        HIPCHK(c, hipMemcpyAsync(nl, c->rec_left, n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nr, c->rec_right, n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nm, c->rec_merged, n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nc, c->rec_count, n * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ns, c->rec_sites, n * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nv, c->rec_live, n * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_records(c);
    c->rec_left = nl; c->rec_right = nr; c->rec_merged = nm; c->rec_count = nc; c->rec_sites = ns; c->rec_live = nv;
    c->rec_cap = ncap;
    return 0;
}

// The head of a training call: the state told what is asked, the results of the last call forgotten.
int train_begin(yabpe_ctx *c, uint32_t num_merges, uint64_t min_frequency, uint32_t *rec_base) {
    TRY(state_pull(c));
    DevState *h = c->st_host;
    *rec_base = h->iter;
    if ((uint64_t)*rec_base + num_merges > 0xFFFFFFF0ull) return fail(c, YABPE_E_CAPACITY, "more than 2^32 merges in one context");
    h->num_merges = *rec_base + num_merges;
    h->min_freq = min_frequency;
    h->done = 0;
    h->halt = 0;
    h->halt_req = 0;
    if (c->id_bits != 32) {  // (the batch the u16 selection keeps; the u32 loop selects one merge per launch)
        h->n_batch = 0;
        h->n_select = 0;
        h->batch_others = 0;
        h->kmax = 1;
        h->win_shift = 3;
    }
    TRY(state_push(c));
    c->rec_n = 0;
    c->log_sites.clear();
    c->log_live.clear();
    c->ev_iter.clear();
    c->ev_us.clear();
    c->ev_scan_us.clear();
    return 0;
}
// ... and its per-merge records: `first` of them, none kept from the last call, no sites counted yet
int train_begin_records(yabpe_ctx *c, uint32_t first) {
    if (c->rec_cap < first) free_records(c);
    TRY(reserve_records(c, first, 0));
    HIPCHK(c, hipMemsetAsync(c->rec_sites, 0, (size_t)c->rec_cap * 8, c->stream));
    return 0;
}
// The tail of a training call: the n merges of the call to the caller's arrays, their site (and live-slot) log to the context.
int train_copy_out(yabpe_ctx *c, uint32_t n, bool live, uint32_t *out_left, uint32_t *out_right, uint32_t *out_merged, uint64_t *out_count,
                   uint32_t *out_n_merges) {
    c->rec_n = n;
    c->log_sites.assign(n, 0);
    c->log_live.assign(n, 0);
    if (n) {
        HIPCHK(c, hipMemcpy(c->log_sites.data(), c->rec_sites, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (live) HIPCHK(c, hipMemcpy(c->log_live.data(), c->rec_live, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (out_left) HIPCHK(c, hipMemcpy(out_left, c->rec_left, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (out_right) HIPCHK(c, hipMemcpy(out_right, c->rec_right, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (out_merged) HIPCHK(c, hipMemcpy(out_merged, c->rec_merged, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (out_count) HIPCHK(c, hipMemcpy(out_count, c->rec_count, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (out_n_merges) *out_n_merges = n;
    return 0;
}
}  // namespace

#include "yabpe_id32_host.h"

// =================================================================================================== C ABI
extern "C" {

// The option "digit_group" (group_logic.h), read by every call that pre-tokenises: 0 (GPT-2's \p{N}+) or G in [1, 255].
static int digit_group_opt(yabpe_ctx *c, uint32_t *G) {
    const int64_t v = optv(c, "digit_group", 0);
    if (v < 0 || v > (int64_t)GRP_MAX) return fail(c, YABPE_E_INVALID, "option digit_group is %lld: 0 (off) or a group of 1 .. 255 digits", (long long)v);
    *G = (uint32_t)v;
    return YABPE_OK;
}

// The option "split_pattern" (split4_logic.h, split5_logic.h), read by every call that pre-tokenises, after digit_group: 0 the
// GPT-2 pattern, 1 the cl100k pattern, 3 the o200k_base pattern; the last two need a digit group for their \p{N}{1,G}.  2 is
// reserved and refused.
static int split_pattern_opt(yabpe_ctx *c, uint32_t G, uint32_t *pattern) {
    const int64_t v = optv(c, "split_pattern", 0);
    if (v != 0 && v != 1 && v != 3)
        return fail(c, YABPE_E_INVALID, "option split_pattern is %lld: 0 (GPT-2), 1 (cl100k) or 3 (o200k_base)", (long long)v);
    if (v && G == 0)
        return fail(c, YABPE_E_INVALID, "option split_pattern is %lld (%s): digit_group must be 1 .. 255, it is 0", (long long)v, v == 1 ? "cl100k" : "o200k_base");
    *pattern = (uint32_t)v;
    return YABPE_OK;
}

// the pre-tokeniser's class of one code point, from the runs the class table is built from
static uint8_t class_of(uint32_t cp) {
    unsigned lo = 0, hi = YB_UNICODE_CLASS_NRUNS; // the last run that starts at or below cp
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) / 2;
        if (YB_UNICODE_CLASS_RUNS[mid][0] <= cp) lo = mid;
        else hi = mid;
    }
    return YB_UNICODE_CLASS_RUNS[lo][0] <= cp ? (uint8_t)YB_UNICODE_CLASS_RUNS[lo][1] : (uint8_t)PT_O;
}

// the class per code point of the pre-tokeniser (unicode_classes.inc expanded), built on first use
static int class_table(yabpe_ctx *c) {
    if (c->pt_cls) return 0;
    std::vector<uint8_t> cls(0x110000, PT_O);
    for (unsigned r = 0; r < YB_UNICODE_CLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_CLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_CLASS_NRUNS ? YB_UNICODE_CLASS_RUNS[r + 1][0] : 0x110000;
        memset(cls.data() + lo, (int)YB_UNICODE_CLASS_RUNS[r][1], hi - lo);
    }
    TRY(dmalloc(c, &c->pt_cls, cls.size()));
    HIPCHK(c, hipMemcpy(c->pt_cls, cls.data(), cls.size(), hipMemcpyHostToDevice));
    return 0;
}

// the table of the o200k_base pattern (class, sub-class, U+0020 / U+002F, CR / LF per code point), built on its first use
static int class_table5(yabpe_ctx *c) {
    if (c->pt_cls5) return 0;
    std::vector<uint8_t> sub(0x110000, 0), cls(0x110000);
    for (unsigned r = 0; r < YB_UNICODE_SUBCLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_SUBCLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_SUBCLASS_NRUNS ? YB_UNICODE_SUBCLASS_RUNS[r + 1][0] : 0x110000;
        memset(sub.data() + lo, (int)YB_UNICODE_SUBCLASS_RUNS[r][1], hi - lo);
    }
    for (unsigned r = 0; r < YB_UNICODE_CLASS_NRUNS; ++r) {
        const unsigned lo = YB_UNICODE_CLASS_RUNS[r][0];
        const unsigned hi = r + 1 < YB_UNICODE_CLASS_NRUNS ? YB_UNICODE_CLASS_RUNS[r + 1][0] : 0x110000;
        for (unsigned cp = lo; cp < hi; ++cp) cls[cp] = pt5_table_entry(cp, (uint8_t)YB_UNICODE_CLASS_RUNS[r][1], sub[cp]);
    }
    TRY(dmalloc(c, &c->pt_cls5, cls.size()));
    HIPCHK(c, hipMemcpy(c->pt_cls5, cls.data(), cls.size(), hipMemcpyHostToDevice));
    return 0;
}

int yabpe_abi_version(void) { return YABPE_ABI_VERSION; }

int yabpe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *yabpe_last_error(const yabpe_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int yabpe_create(yabpe_ctx **out, int device_id) {
    if (!out) return fail(nullptr, YABPE_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, YABPE_E_NODEVICE, "no HIP device available (%s); the BPE hot path has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device_id < 0 || device_id >= n) return fail(nullptr, YABPE_E_INVALID, "device_id %d out of range [0,%d)", device_id, n);
    yabpe_ctx *c = new yabpe_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) {
        delete c;
        return fail(nullptr, YABPE_E_HIP, "hipSetDevice(%d) failed", device_id);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        // The streaming-phase grid must be resident all at once: its workgroups stride over the tiles and all finish together, so
        // a workgroup that has to wait for a free slot runs alone afterwards (5 per CU asked, 4 resident: +25 % on every launch).
        int occ = 0, lo = 1 << 30;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_apply<false, false>, BLOCK, 0) == hipSuccess && occ > 0) lo = std::min(lo, occ);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_apply<false, true>, BLOCK, 0) == hipSuccess && occ > 0) lo = std::min(lo, occ);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_apply<true, false>, BLOCK, 0) == hipSuccess && occ > 0) lo = std::min(lo, occ);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_count<false>, BLOCK, 0) == hipSuccess && occ > 0) lo = std::min(lo, occ);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_count<true>, BLOCK, 0) == hipSuccess && occ > 0) lo = std::min(lo, occ);
        (void)hipGetLastError();
        c->apply_occ = lo == (1 << 30) ? 4 : lo;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&c->st, sizeof(DevState)) != hipSuccess ||
        hipHostMalloc((void **)&c->st_host, sizeof(DevState), hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&c->scratch64, 16 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void **)&c->blk_stats, 2 * MAX_APPLY_BLOCKS * sizeof(unsigned long long)) != hipSuccess) {
        int code = fail(nullptr, YABPE_E_HIP, "context allocation failed: %s", hipGetErrorString(hipGetLastError()));
        yabpe_destroy(c);
        return code;
    }
    (void)hipMemset(c->st, 0, sizeof(DevState));
    (void)hipMemset(c->blk_stats, 0, 2 * MAX_APPLY_BLOCKS * sizeof(unsigned long long));
    memset(c->st_host, 0, sizeof(DevState));
    *out = c;
    return YABPE_OK;
}

void yabpe_destroy(yabpe_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    yabpe_synth_free(c);
    yabpe_pretokenize_free(c);
    yabpe_encode_free(c);
    dfree(c->enc_keys); dfree(c->enc_vals); dfree(c->enc_out_id);
    dfree(c->enc_sp_bytes); dfree(c->enc_sp_has); dfree(c->enc_sp_off); dfree(c->enc_sp_id);
    for (auto &e : c->enc_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_decode_free(c);
    dfree(c->dec_ent); dfree(c->dec_pool);
    for (auto &e : c->dec_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_layout_free(c);
    for (auto &e : c->lay_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_mask_free(c);
    for (auto &e : c->mask_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_span_free(c);
    for (auto &e : c->span_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_fim_free(c);
    for (auto &e : c->fim_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_pool_clear(c);
    for (auto &e : c->wpool_ev)
        if (e) (void)hipEventDestroy(e);
    dfree(c->pt_cls);
    dfree(c->pt_cls5);
    yabpe_normalize_free(c);
    dfree(c->nfc_prop); dfree(c->nfc_decomp); dfree(c->nfc_pairs);
    for (auto &e : c->norm_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_utf8_repair_free(c);
    for (auto &e : c->utf8_ev)
        if (e) (void)hipEventDestroy(e);
    yabpe_lowercase_free(c);
    dfree(c->case_tab);
    for (auto &e : c->case_ev)
        if (e) (void)hipEventDestroy(e);
    free_corpus(c);
    id32_free_corpus(c);
    dfree(c->partials32);
    dfree(c->cand32_state);
    dfree(c->cand32_list);
    free_records(c);
    dfree(c->tt.pool); dfree(c->tt.off); dfree(c->tt.len); dfree(c->tt.rec); dfree(c->tt.vset);
    dfree(c->partials);
    dfree(c->st);
    dfree(c->scratch64);
    dfree(c->blk_stats);
    dfree(c->blk_read);
    dfree(c->cand_state);
    dfree(c->sel_ticket);
    dfree(c->cand);
    dfree(c->cand_bits);
    dfree(c->xsend);
    dfree(c->xrecv);
    dfree(c->xsmall);
    p2p_close(c);
    if (c->p2p_e0) (void)hipEventDestroy(c->p2p_e0);
    if (c->p2p_e1) (void)hipEventDestroy(c->p2p_e1);
    if (c->comm && rccl()) (void)rccl()->CommDestroy(c->comm);
    if (c->st_host) (void)hipHostFree(c->st_host);
    for (auto &e : c->events) {
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
        (void)hipEventDestroy(e.e2);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int yabpe_set_option(yabpe_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return YABPE_E_INVALID;
    if (strcmp(name, "id_bits") == 0) {  // the id width of the merge loop: read by yabpe_set_vocab, fixed from then on
        if (value != 16 && value != 32) return fail(c, YABPE_E_INVALID, "option id_bits is %lld: 16 or 32", (long long)value);
        if (c->id_bits_fixed && value != c->id_bits)
            return fail(c, YABPE_E_INVALID, "option id_bits cannot change after yabpe_set_vocab (it is %d)", c->id_bits);
        if (value == 32 && c->multi) return fail(c, YABPE_E_INVALID, "id_bits = 32 is single-device: this context has a communicator attached");
        if (!c->id_bits_fixed) c->id_bits = (int)value;
    }
    c->opt[name] = value;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- vocab
int yabpe_set_vocab(yabpe_ctx *c, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tokens) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!tok_bytes || !tok_off || n_tokens < 256) return fail(c, YABPE_E_INVALID, "vocab needs the 256 byte tokens first");
    for (uint32_t b = 0; b < 256; ++b)
        if (tok_off[b + 1] - tok_off[b] != 1 || tok_bytes[tok_off[b]] != b)
            return fail(c, YABPE_E_INVALID, "token %u must be the single byte %u (trainer.py:123-125)", b, b);
    if (c->id_bits == 32) return id32_set_vocab(c, tok_bytes, tok_off, n_tokens);
    if (n_tokens >= YB_MAX_TOKENS) return fail(c, YABPE_E_CAPACITY, "base vocabulary too large for u16 token ids");
    // the u16 side: fixed capacities (every id, a set of 2^18 slots), the base vocabulary in at most half the pool, lexranks
    const uint32_t pool_cap = (uint32_t)optv(c, "pool_bytes", 64 << 20) & ~3u;
    BaseVocab V;
    base_vocab_pack(tok_bytes, tok_off, n_tokens, V);
    if (V.pool.size() > pool_cap / 2) return fail(c, YABPE_E_CAPACITY, "base vocabulary bytes exceed the token pool");
    TRY(base_vocab_index(c, V));
    for (uint32_t r = 0; r < n_tokens; ++r) V.rec[V.order[r]].rank = r;
    return base_vocab_upload(c, V, pool_cap, YB_MAX_TOKENS, 1u << 18);
}

// ---------------------------------------------------------------------------------------------- corpus
int yabpe_load_words(yabpe_ctx *c, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq,
                     uint64_t n_words, uint32_t flags) {
    if (!c) return YABPE_E_INVALID;
    if (c->id_bits == 32) return id32_load(c, bytes, word_off, word_freq, n_words, flags, nullptr, nullptr, nullptr, 0);
    return load_words_impl(c, bytes, word_off, word_freq, n_words, flags, nullptr);
}

int yabpe_load_words_resumed(yabpe_ctx *c, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words,
                             uint32_t flags, const uint32_t *merge_left, const uint32_t *merge_right, const uint32_t *merge_merged,
                             uint32_t n_merges) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_vocab) return fail(c, YABPE_E_INVALID, "call yabpe_set_vocab first (with all of the model's tokens)");
    if (c->id_bits == 32) {
        if (n_merges && !word_freq && !(flags & YABPE_LOAD_DEDUP))
            return fail(c, YABPE_E_INVALID, "a resumed load needs the pooled layout: pass word_freq or YABPE_LOAD_DEDUP");
        return id32_load(c, bytes, word_off, word_freq, n_words, flags, merge_left, merge_right, merge_merged, n_merges);
    }
    if (n_merges == 0) return load_words_impl(c, bytes, word_off, word_freq, n_words, flags, nullptr);
    if (!word_freq && !(flags & YABPE_LOAD_DEDUP))
        return fail(c, YABPE_E_INVALID, "a resumed load needs the pooled layout: pass word_freq or YABPE_LOAD_DEDUP");
    if (c->multi) return fail(c, YABPE_E_INVALID, "a resumed load on several GPUs is not supported");
    if (!merge_left || !merge_right || !merge_merged) return fail(c, YABPE_E_INVALID, "merge triples are NULL");
    TRY(check_merge_triples(c, merge_left, merge_right, merge_merged, n_merges));
    RpTableHost th;
    rp_build_table(merge_left, merge_right, merge_merged, n_merges, &th);
    Scratch S(c->device, c->rank);
    RpTable t{};
    TRY(rp_upload(c, S, th, &t));
    const int rc = load_words_impl(c, bytes, word_off, word_freq, n_words, flags, &t);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int yabpe_resume_stats(yabpe_ctx *c, yabpe_resume_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->resume_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- train
static SelectParams select_params(yabpe_ctx *c, uint32_t rec_base, uint32_t n_part, uint32_t n_blk) {
    return SelectParams{c->partials, n_part, c->tt, c->st, c->rec_left, c->rec_right, c->rec_merged,
                        c->rec_count, c->rec_sites, c->rec_live, rec_base, c->table,
                        c->multi ? reinterpret_cast<DeltaHdr *>(c->xsend) : nullptr, c->blk_stats, std::max(n_blk, 1u),
                        c->use_cand ? c->cand_state : nullptr, (!c->weighted && !c->multi) ? 1u : 0u};
}

// The selection as launches of its own (trainer.py:241-251, 296-300): exact argmax over the candidate list, or over the
// whole table when there is no list, then stop rules and merged-token creation.  Selects ONE merge.
static int launch_select(yabpe_ctx *c, uint32_t rec_base) {
    const uint32_t n_part = c->use_cand ? std::min<uint32_t>(c->n_partials_cap, 64) : c->n_partials;
    const SelectParams S = select_params(c, rec_base, n_part, c->blk_used);
    c->blk_used = 0;  // the selection folds and clears them; what follows counts the next merge's grids
    if (c->use_cand) {  // (its last workgroup selects)
        CandParams CP{c->table, c->tt.rec, c->partials, c->st, c->cand_state, c->sel_ticket, S};
        hipLaunchKernelGGL(k_argmax_cand, dim3(n_part), dim3(BLOCK), 0, c->stream, CP);
    } else {
        ArgmaxParams A{c->table, c->tt.rec, c->partials, c->st};
        hipLaunchKernelGGL(k_argmax_partial, dim3(c->n_partials), dim3(BLOCK), 0, c->stream, A);
        hipLaunchKernelGGL(k_select, dim3(1), dim3(BLOCK), 0, c->stream, S);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- the u16 merge loop's driver: one run state, the launches, the steps of a round (the decisions are train_rules.h's)
extern "C++" {
namespace {

// Every option the loop reads, looked up once at the top of the call.  An option cannot change during a call (one thread,
// one context), so reading it here and not at every launch changes no behaviour.
struct TrainOpts {
    uint32_t check, ev_sample, ev_sample_dense;
    uint64_t retile_min_tiles;
    int64_t retile_pct, split, split_pct, batch_max, cand_rebuild_every, cand_target, sig_rebuild_every, sig_rebuild_pct;
    int64_t apply_blocks, full_wpb, wide_sites_per_cu, full_skip_blocks, chunk_steal, agg_small;
    int64_t delta_granule, delta_headroom_pct, delta_margin, delta_floor, p2p_timeout_ms, table_load_pct, table_grow_x;
    bool trace_host, trace_exchange, fused, rank_rides, hist, delta_adapt;
};
TrainOpts train_opts(yabpe_ctx *c) {
    TrainOpts O{};
    O.check = (uint32_t)std::max<int64_t>(1, optv(c, "check_interval", 32));
    O.ev_sample = (uint32_t)std::max<int64_t>(0, optv(c, "event_sample", 0));
    O.ev_sample_dense = (uint32_t)std::max<int64_t>(0, optv(c, "event_sample_dense", (int64_t)O.ev_sample));  // fused k_apply launches
    O.retile_min_tiles = (uint64_t)optv(c, "retile_min_tiles", 4096);
    O.retile_pct = optv(c, "retile_pct", 60);
    O.split = optv(c, "split", -1);
    O.split_pct = optv(c, "split_pct", 100);
    O.batch_max = optv(c, "batch_max", KMAX);
    O.cand_rebuild_every = optv(c, "cand_rebuild_every", 512);
    O.cand_target = optv(c, "cand_target", 768);
    O.sig_rebuild_every = optv(c, "sig_rebuild_every", 16384);
    O.sig_rebuild_pct = optv(c, "sig_rebuild_pct", 20);
    O.apply_blocks = optv(c, "apply_blocks", OPT_UNSET);
    O.full_wpb = optv(c, "full_wpb", 0);
    O.wide_sites_per_cu = optv(c, "wide_sites_per_cu", 20);
    O.full_skip_blocks = optv(c, "full_skip_blocks", OPT_UNSET);
    O.chunk_steal = optv(c, "chunk_steal", 1);
    O.agg_small = optv(c, "agg_small", 1);
    O.delta_granule = optv(c, "delta_granule", 1024);
    O.delta_headroom_pct = optv(c, "delta_headroom_pct", 200);
    O.delta_margin = optv(c, "delta_margin", 1024);
    O.delta_floor = optv(c, "delta_floor", 2048);
    O.p2p_timeout_ms = optv(c, "p2p_timeout_ms", 20000);
    O.table_load_pct = optv(c, "table_load_pct", 30);
    O.table_grow_x = optv(c, "table_grow_x", 8);
    O.trace_host = optv(c, "trace_host", 0) != 0;  // (debugging a stuck multi-GPU job: where is this rank's host?)
    O.trace_exchange = optv(c, "trace_exchange", 0) != 0;
    O.fused = optv(c, "fused", 1) != 0;
    O.rank_rides = optv(c, "rank_rides", 1) != 0;
    O.hist = optv(c, "hist", 1) != 0;
    O.delta_adapt = optv(c, "delta_adapt", 1) != 0;
    return O;
}

struct TrainRun {
    yabpe_ctx *c;
    DevState *h;  // the pinned copy of the device state, as of the last pull
    TrainOpts O;
    uint32_t num_merges, rec_base;
    // progress
    uint32_t i = 0;  // merges selected so far in this call (read back from the device between rounds of launches)
    bool first_round = true;
    bool skip_cand_once = false;  // the last round hit HALT_RESCAN: finish its merge with the full scan
    // form of this round
    bool sparse_global = false;  // the sparse form has been called for (by any rank)
    bool sparse_now = false, fuse = false;
    uint32_t kmax = 1, n_launch = 0, apply_grid = 0;
    // candidate list
    unsigned long long prev_best = 0;
    uint32_t cand_n_all = 0;  // length of the list at the last read (multi-GPU: of the longest replica's)
    // measurement marks: where the sparse phase and the second half of the call's merges begin
    Events<4> ev;  // start, end, split, tail
    bool split_marked = false, tail_marked = false;
    uint32_t split_at = 0, tail_at = 0;
    uint32_t dense_applied = 0;  // merges the streaming launches applied (what was selected when the form changed, less the pending batch)
    uint64_t launches_sparse = 0, launches_at_tail = 0, launches_dense = 0;
    uint64_t tokens_at_start = 0;
    // event sampling
    size_t ev_next = 0;
    uint64_t launch_no = 0;
};
enum RoundNext { ROUND_NEXT, ROUND_AGAIN, ROUND_STOP };

__attribute__((format(printf, 2, 3))) void trace(const TrainRun &R, const char *fmt, ...) {
    if (!R.O.trace_host) return;
    fprintf(stderr, "[yabpe r%d] ", R.c->rank);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    fflush(stderr);
}

// the event pair of every Nth LAUNCH (iter_rel: the merges selected so far, a lower bound in the fused forms), else NULL
EventPair *sample_launch(TrainRun &R, uint32_t iter_rel) {
    yabpe_ctx *c = R.c;
    const uint32_t every = c->split_mode ? R.O.ev_sample : R.O.ev_sample_dense;
    if (!every || (R.launch_no++ % every) != 0) return nullptr;
    if (R.ev_next == c->events.size()) {
        EventPair n{};
        if (hipEventCreate(&n.e0) != hipSuccess || hipEventCreate(&n.e1) != hipSuccess || hipEventCreate(&n.e2) != hipSuccess) return nullptr;
        c->events.push_back(n);
    }
    c->events[R.ev_next].iter_rel = iter_rel;
    return &c->events[R.ev_next++];
}
// the launches from merge i on did nothing: timed again in the re-run
void unsample_from(TrainRun &R) {
    while (R.ev_next > 0 && R.c->events[R.ev_next - 1].iter_rel >= R.i) --R.ev_next;
}

// Can the apply launch of the merges that are selected now end with the selection of the next ones?
bool can_fuse(const TrainRun &R) {
    const yabpe_ctx *c = R.c;
    if (!c->use_cand || !R.O.fused) return false;
    if (c->multi) return true;        // the selection rides on the launch that applies the exchanged records (k_delta_apply)
    if (!c->n_tiles) return false;
    if (!c->split_mode) return true;  // k_apply
    return c->sig && c->sig_valid;    // k_scan_skip
}

// What the launches that apply one selection share.
struct ApplyJob {
    RankParams rank;
    uint32_t rank_blocks;  // workgroups of the lexrank maintenance ...
    bool rank_rides;       // ... riding on the launch over the tiles as extra workgroups
    PairTable out_table;   // where the pair-count updates go: the pair table, or (multi-GPU) this rank's send buffer as records
    bool fuse;             // the launch that finishes the apply also selects the next merges (its last workgroup: fused_select_tail)
    bool fuse_kernel;      // ... and that launch is the one over the tiles (single GPU)
    LongParams LW;
    uint32_t long_group, long_blocks;  // long words per workgroup; workgroups of theirs riding like the lexranks (0: launched on their own)
    uint32_t rr_blocks() const { return rank_rides ? rank_blocks : 0u; }
};
// the fused selection folds the per-workgroup counters of THIS launch too: it must know the larger grid
FuseParams fuse_params(const TrainRun &R, const ApplyJob &J, uint32_t grid_now) {
    FuseParams F{};
    if (J.fuse_kernel) {
        F.ticket = R.c->sel_ticket;
        F.sel = select_params(R.c, R.rec_base, 0u, std::max(R.c->blk_used, grid_now));
    }
    return F;
}
ApplyParams apply_params(const yabpe_ctx *c, const ApplyJob &J) {
    return ApplyParams{c->tiles, c->tile_len, c->tile_wbase, c->wfreq, c->n_tiles, J.out_table, c->st, c->blk_stats,
                       c->split_mode ? c->sig : nullptr, c->sig_stride, (uint32_t)AGG_N - 1u, 1u};  // signatures are maintained in the sparse form only
}

// streaming form: one merge per launch, one coalesced pass over the live stream
int launch_streaming(TrainRun &R, const ApplyJob &J, uint32_t tokens_upper) {
    yabpe_ctx *c = R.c;
    const ApplyParams P = apply_params(c, J);
    const uint32_t apply_grid = R.apply_grid;
    const FuseParams F = fuse_params(R, J, apply_grid);
    const uint32_t long_first = apply_grid + J.rr_blocks(), grid = long_first + J.long_blocks;
    c->blk_used = std::max(c->blk_used, apply_grid);
    if (c->weighted)
        hipLaunchKernelGGL(k_apply<true>, dim3(grid), dim3(BLOCK), 0, c->stream, P, apply_grid, J.rank, F, J.LW, long_first);
    else if (R.O.hist && tokens_upper <= (uint32_t)HIST_V)  // (every token id this launch can meet indexes the direct store)
        hipLaunchKernelGGL((k_apply<false, true>), dim3(grid), dim3(BLOCK), 0, c->stream, P, apply_grid, J.rank, F, J.LW, long_first);
    else
        hipLaunchKernelGGL(k_apply<false>, dim3(grid), dim3(BLOCK), 0, c->stream, P, apply_grid, J.rank, F, J.LW, long_first);
    return 0;
}

template <int NW>
void launch_scan_skip(yabpe_ctx *c, uint32_t grid, const ScanSkipParams &SQ) {
    if (c->weighted)
        hipLaunchKernelGGL((k_scan_skip<true, NW>), dim3(grid), dim3(NW * 64), 0, c->stream, c->st, SQ);
    else
        hipLaunchKernelGGL((k_scan_skip<false, NW>), dim3(grid), dim3(NW * 64), 0, c->stream, c->st, SQ);
}
// sparse form: skip index + rewrite of the tiles that pass, a batch of merges per launch (the shape: sparse_geom_rule)
int launch_sparse(TrainRun &R, const ApplyJob &J) {
    yabpe_ctx *c = R.c;
    const TrainOpts &O = R.O;
    if (!(c->sig && c->sig_valid)) return fail(c, YABPE_E_INTERNAL, "sparse form without signatures");
    const SparseGeom g = sparse_geom_rule(c->n_tiles, (uint32_t)c->n_cu, c->st_host->best_count, c->weighted, c->kmax_now, O.full_wpb,
                                          O.wide_sites_per_cu, O.full_skip_blocks, O.chunk_steal, O.agg_small);
    if (!c->blk_read) {
        TRY(dmalloc(c, &c->blk_read, BLK_READ_WORDS));
        HIPCHK(c, hipMemsetAsync(c->blk_read, 0, BLK_READ_WORDS * 8, c->stream));
    }
    ApplyParams P = apply_params(c, J);
    P.agg_mask = g.agg_mask;
    const ScanSkipParams SQ{P, c->blk_read, g.scan_grid, g.kt, g.chunk, J.rank, fuse_params(R, J, g.scan_grid), J.LW, g.scan_grid + J.rr_blocks(),
                            g.piece, g.n_pieces, g.pieces ? c->blk_read + 2 * MAX_LISTS : nullptr,
                            g.pieces ? ++c->piece_tag : 0ull, c->blk_read + MAX_LISTS};
    c->blk_used = std::max(c->blk_used, g.scan_grid);
    const uint32_t grid = g.scan_grid + J.rr_blocks() + J.long_blocks;
    if (g.nw == 16) launch_scan_skip<16>(c, grid, SQ);
    else launch_scan_skip<8>(c, grid, SQ);
    c->scan_skip_launches++;
    return 0;
}

// Multi-GPU, per batch: the apply launch left this rank's updates as [header | records] in its send buffer (the aggregator
// flush writes them there: no delta table, no extraction pass); ONE all-gather; ONE launch adds every rank's records to
// the replica and -- fused form -- selects the next merges in its last workgroup.
int launch_exchange(TrainRun &R, const ApplyJob &J) {
    yabpe_ctx *c = R.c;
    const uint64_t xbytes = 16 + (uint64_t)c->xeff * sizeof(DeltaRec);  // [header | xeff records] per rank, packed at that stride
    const uint8_t *recv = c->xrecv;
    uint64_t rstride = xbytes;
    if (c->p2p) {  // push into the peers' memory, wait for theirs: one small launch, no collective
        XchgParams X{};
        X.send = c->xsend;
        for (int r = 0; r < c->n_ranks; ++r) X.peer[r] = c->p2p_peer[r];
        X.flags_off = c->p2p_flags_off;
        X.half_bytes = c->p2p_half;
        X.stride = c->p2p_stride;
        X.seq = ++c->p2p_seq;
        X.rank = (uint32_t)c->rank;
        X.n_ranks = (uint32_t)c->n_ranks;
        X.cap = c->xeff;
        X.timeout_ticks = (unsigned long long)R.O.p2p_timeout_ms * 100000ull;
        X.st = c->st;
        const bool timed = !c->p2p_pending && c->p2p_e0;  // (one exchange per round of launches is timed)
        if (timed) HIPCHK(c, hipEventRecord(c->p2p_e0, c->stream));
        hipLaunchKernelGGL(k_xchg_push, dim3((uint32_t)c->n_ranks), dim3(BLOCK), 0, c->stream, X);
        if (timed) {
            HIPCHK(c, hipEventRecord(c->p2p_e1, c->stream));
            c->p2p_pending = true;  // (read at the end of this round of launches)
        }
        recv = c->p2p_area + (X.seq & 1ull) * c->p2p_half;
        rstride = c->p2p_stride;
    } else {
        TRY(comm_allgather(c, c->xsend, c->xrecv, xbytes));
    }
    c->xeff_sum += c->xeff;
    DeltaApplyParams DA{recv, (uint32_t)c->n_ranks, c->xeff, rstride, c->table, c->st, FuseParams{}, c->p2p ? 1u : 0u};
    if (J.fuse) {
        DA.F.ticket = c->sel_ticket;
        DA.F.sel = select_params(c, R.rec_base, 0u, c->blk_used);
    }
    hipLaunchKernelGGL(k_delta_apply, dim3(cdiv64((uint64_t)c->n_ranks * c->xeff, DELTA_RPW)), dim3(BLOCK), 0, c->stream, DA);
    c->exchanges++;
    return 0;
}

// Applies the selected merges (DevState::batch) to the token stream and the pair table (trainer.py:254-294): the lexranks
// and the long words (more than 63 tokens: outside the tile stream) ride on the launch over the tiles where there is one,
// else they are launched on their own; then the exchange.  fuse: one launch per batch, see ApplyJob.
int launch_merges(TrainRun &R, uint32_t tokens_upper, EventPair *ev, bool fuse) {
    yabpe_ctx *c = R.c;
    ApplyJob J{};
    J.rank = RankParams{c->tt, c->st};
    J.rank_blocks = cdiv64(std::min<uint32_t>(tokens_upper, YB_MAX_TOKENS), BLOCK);
    const bool sparse = c->split_mode && c->sig && c->sig_valid;
    J.rank_rides = c->n_tiles && (fuse || R.O.rank_rides) && (c->split_mode ? sparse : true);
    if (!J.rank_rides) hipLaunchKernelGGL(k_rank_update, dim3(J.rank_blocks), dim3(BLOCK), 0, c->stream, J.rank);
    J.out_table = c->table;
    if (c->multi) {
        J.out_table = PairTable{};
        J.out_table.sink_hdr = reinterpret_cast<DeltaHdr *>(c->xsend);
        J.out_table.sink_rec = reinterpret_cast<DeltaRec *>(c->xsend + 16);
        J.out_table.sink_cap = c->xeff;  // (what this exchange transmits: a rank with more records than that reports it by its count)
    }
    J.fuse = fuse;
    J.fuse_kernel = fuse && !c->multi;
    if (ev) {
        ev->split = c->split_mode;
        HIPCHK(c, hipEventRecord(ev->e0, c->stream));
    }
    // one signature word per long word and merge, the few words that pass are rewritten
    // (words per workgroup: about two workgroups per CU while there are few long words, BLOCK when there are many)
    J.long_group = (uint32_t)std::min<uint64_t>(BLOCK, std::max<uint64_t>(32, cdiv64(c->n_long, 2ull * std::max(1, c->n_cu))));
    J.LW = LongParams{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, J.out_table, c->st, c->long_sig, c->long_sig_stride, J.long_group};
    const bool long_rides = J.fuse_kernel && c->n_long && c->n_tiles && J.rank_rides;
    J.long_blocks = long_rides ? cdiv64(c->n_long, J.long_group) : 0u;
    if (J.fuse_kernel && c->n_long && !long_rides)  // (no tile launch to ride on: on their own, first -- the fused launch must be the last one to touch the table)
        hipLaunchKernelGGL(k_apply_long, dim3(cdiv64(c->n_long, J.long_group)), dim3(BLOCK), 0, c->stream, J.LW);
    if (c->n_tiles) TRY(c->split_mode ? launch_sparse(R, J) : launch_streaming(R, J, tokens_upper));
    if (ev) {
        HIPCHK(c, hipEventRecord(ev->e1, c->stream));
        HIPCHK(c, hipEventRecord(ev->e2, c->stream));
    }
    if (!J.fuse_kernel && c->n_long) hipLaunchKernelGGL(k_apply_long, dim3(cdiv64(c->n_long, J.long_group)), dim3(BLOCK), 0, c->stream, J.LW);
    if (c->multi) TRY(launch_exchange(R, J));
    if (fuse) {
        c->blk_used = 0;  // folded by the selection at the end of that launch
        c->fused_launches++;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- a round: prepare, launch, read, recover, housekeeping
// The argmax grid sized to the table, the form, the measurement marks, the candidate list and the signatures kept up, the
// batch limit on the device, records for everything the round can select.
int round_prepare(TrainRun &R) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    const TrainOpts &O = R.O;
    const uint32_t i = R.i;
    const uint32_t want_partials = partials_rule(c->table_cap);
    if (want_partials != c->n_partials) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->partials);
        c->partials = nullptr;
        c->n_partials_cap = std::max<uint32_t>(want_partials, 64);
        TRY(dmalloc(c, &c->partials, c->n_partials_cap));
        c->n_partials = want_partials;
    }
    R.apply_grid = count_grid_rule(c->n_tiles, (uint32_t)c->n_cu, (uint32_t)c->apply_occ, O.apply_blocks);
    R.sparse_now = sparse_now_rule(O.split, R.sparse_global);
    c->split_mode = R.sparse_now && c->n_tiles;  // (a rank without tiles launches no apply kernel, but selects like the others)
    if (!R.tail_marked && i >= R.num_merges / 2) {
        R.tail_marked = true;
        R.tail_at = i;
        R.launches_at_tail = R.launches_sparse;
        HIPCHK(c, hipEventRecord(R.ev.e[3], c->stream));
    }
    if (c->split_mode && !R.split_marked) {
        R.split_marked = true;
        R.split_at = i;
        R.dense_applied = i - std::min<uint32_t>(i, c->pending ? h->n_batch : 0u);
        R.launches_dense = h->n_select - std::min<uint32_t>(h->n_select, c->pending ? 1u : 0u);  // (selections that committed a batch = launches with work; launches queued behind a stop flag return at once)
        HIPCHK(c, hipEventRecord(R.ev.e[2], c->stream));
    }
    if (R.skip_cand_once) {
        c->use_cand = false;
        R.skip_cand_once = false;
    } else if (h->iter > R.rec_base) {
        if (cand_rebuild_rule(c->use_cand, i, c->cand_built_at, O.cand_rebuild_every, h->best_count, c->table.cand_T, R.prev_best, R.cand_n_all, O.cand_target)) {
            trace(R, "cand_rebuild at %u", i);
            TRY(cand_rebuild(c, h->best_count));
            c->cand_built_at = i;
            c->cand_best_at_build = h->best_count;
        }
        R.prev_best = h->best_count;
    }
    if (c->split_mode && sig_rebuild_rule(c->sig_valid, i, c->sig_built_at, O.sig_rebuild_every, c->sig_tokens_at_build, h->tokens_now, O.sig_rebuild_pct)) {
        trace(R, "build_signatures at %u", i);
        TRY(build_signatures(c));
        c->sig_valid = true;
        c->sig_built_at = i;
    }
    R.kmax = round_kmax_rule(R.sparse_now, O.batch_max);
    if (R.kmax != c->kmax_now) {
        HIPCHK(c, hipMemcpyAsync(&c->st->kmax, &R.kmax, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        c->kmax_now = R.kmax;
        h->kmax = R.kmax;
    }
    R.n_launch = round_launches_rule(R.first_round, R.sparse_now, O.check);
    R.first_round = false;
    TRY(reserve_records(c, round_records_rule(R.num_merges, i, R.n_launch, R.kmax), i));
    return 0;
}

// Fused form: one launch applies the pending merges and selects the next ones; otherwise a merge is a selection launch
// followed by its apply launch(es).  `i` counts selected merges exactly while one launch selects one merge (streaming
// form, unfused); in the sparse form a launch selects a batch and `i` is a lower bound until the next read.
int round_launch(TrainRun &R) {
    yabpe_ctx *c = R.c;
    const uint32_t num_merges = R.num_merges, kmax = R.kmax;
    uint32_t &i = R.i;
    const bool fuse = R.fuse = can_fuse(R);
    const uint32_t tok_upper0 = R.h->n_tokens;
    uint32_t launched = 0;
    if (c->pending && !fuse) {  // leave the fused form: the selected merges are applied on their own
        TRY(launch_merges(R, tok_upper0 + kmax, sample_launch(R, i ? i - 1 : 0), false));
        c->pending = false;
    }
    if (fuse && !c->pending && i < num_merges) {  // enter it: a selection on its own
        TRY(launch_select(c, R.rec_base));
        c->pending = true;
        ++i;
    }
    for (uint32_t l = 0; l < R.n_launch && i < num_merges + (fuse ? 1u : 0u); ++l) {
        ++launched;
        const uint32_t tok_upper = tok_upper_rule(tok_upper0, launched, kmax);
        if (fuse) {
            // (i == num_merges: every merge is selected, the last ones are pending -- this launch applies them and its
            // selection finds the limit reached: done.  An apply launch must never run twice on one selection: in the
            // multi-GPU form the send buffer would still hold the records of the first time.)
            const bool last = i >= num_merges;
            TRY(launch_merges(R, tok_upper, sample_launch(R, i - 1), true));
            if (kmax == 1) ++i; else if (R.sparse_now) ++R.launches_sparse;  // (a batch per launch: i stays a lower bound until the next read)
            if (last) break;
        } else {
            TRY(launch_select(c, R.rec_base));
            TRY(launch_merges(R, tok_upper, sample_launch(R, i), false));
            ++i;
        }
    }
    trace(R, "round of %u launches queued (p2p seq %llu), waiting", launched, (unsigned long long)c->p2p_seq);
    return 0;
}

// What the device really did: the state, the timed exchange, the next exchange's size, this shard's wish for the sparse
// form -- and (multi-GPU) the ranks' agreement on all of it.
int round_read(TrainRun &R) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    const TrainOpts &O = R.O;
    TRY(fold_stats(c));
    TRY(state_pull(c));
    R.i = h->iter - R.rec_base;
    trace(R, "round done: %u merges, halt %u req %u done %u", R.i, h->halt, h->halt_req, h->done);
    if (c->p2p_pending) {  // (the stream is idle: the pair has completed)
        float xms = 0;
        if (hipEventElapsedTime(&xms, c->p2p_e0, c->p2p_e1) == hipSuccess) {
            c->stats.exchange_ms_sampled += xms;
            c->stats.exchanges_sampled += 1;
        } else {
            (void)hipGetLastError();
        }
        c->p2p_pending = false;
    }
    if (h->halt_req && !h->halt) h->halt = h->halt_req;  // raised by the last apply of the batch
    if (h->done || h->halt) c->pending = false;          // the last selection of the batch did not select
    if (c->multi && c->xrecv) {
        // what the exchanges of this round really carried (the largest count of any rank, the same number on every rank)
        const uint32_t seen = h->xmax;
        c->exchange_max_records = std::max<uint64_t>(c->exchange_max_records, seen);
        c->xseen[3] = c->xseen[2]; c->xseen[2] = c->xseen[1]; c->xseen[1] = c->xseen[0]; c->xseen[0] = seen;
        // (nothing shrinks during the first rounds of a job, whose merges differ most from one another)
        if (O.delta_adapt && h->halt != HALT_DELTA_FULL && h->iter - R.rec_base >= 4 * O.check)
            c->xeff = xeff_next_rule(c->xseen, c->xcap, O.delta_headroom_pct, O.delta_margin, O.delta_granule, O.delta_floor);
        if (O.trace_exchange && c->rank == 0) fprintf(stderr, "[yabpe] exchange: merges %u records<= %u next %u halt %u\n", h->iter - R.rec_base, seen, c->xeff, h->halt);
        HIPCHK(c, hipMemsetAsync(&c->st->xmax, 0, sizeof(uint32_t), c->stream));
        h->xmax = 0;
    }
    R.cand_n_all = h->cand_n;
    unsigned long long want_sparse = want_sparse_rule(c->n_tiles, h->iter > R.rec_base, c->weighted, h->sites, h->best_count, O.split_pct) ? 1 : 0;
    if (c->multi) {  // replicas must be in lockstep: same merge count, same flags
        unsigned long long sig = ((unsigned long long)h->iter << 8) | (h->done ? 1u : 0u) | ((unsigned long long)(h->halt & 0x3f) << 1);
        // ... and agree on what must not differ between them: the batch limit follows the form (any rank sparse: all of
        // them), the candidate list is rebuilt for the longest replica's length
        unsigned long long v[3] = {sig, h->cand_n, want_sparse};
        trace(R, "comm_max3");
        TRY(comm_max3(c, v));
        trace(R, "comm_max3 back");
        if (v[0] != sig) return fail(c, YABPE_E_COMM, "ranks diverged (iter/flags %llx vs max %llx)", sig, v[0]);
        R.cand_n_all = (uint32_t)v[1];
        want_sparse = v[2];
    }
    if (want_sparse) R.sparse_global = true;
    return 0;
}

// Services a halt.  *next: run the round again (after a repair), stop (the call's merges are done), or go on.
int round_recover(TrainRun &R, RoundNext *next) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    *next = ROUND_AGAIN;
    if (h->halt == HALT_RESCAN) {  // the candidate set could not prove the maximum: redo that merge with the full scan
        h->halt = 0; h->halt_req = 0;
        TRY(state_push(c));
        c->cand_rescans++;
        R.skip_cand_once = true;
        unsample_from(R);
        return 0;
    }
    if (h->halt == HALT_TABLE_FULL || h->halt == HALT_DELTA_FULL) {
        // the streams are consistent (the apply pass finished everywhere); only table updates were lost:
        // rebuild the table from the token streams, bigger
        const bool delta_full = h->halt == HALT_DELTA_FULL;
        h->halt = 0; h->halt_req = 0;
        TRY(state_push(c));
        if (delta_full) {
            if (c->xeff < c->xcap) {
                c->xeff = xeff_after_full_rule(c->xeff, c->xcap);  // (the buffers hold more: no reallocation)
            } else {
                trace(R, "comm_buffers %u -> %u", c->xcap, c->xcap * 4);
                TRY(comm_buffers(c, c->xcap * 4));
            }
            c->exchange_growths++;
        }
        trace(R, "table_rebuild (delta_full %d)", (int)delta_full);
        TRY(table_rebuild(c, delta_full ? c->table_cap : c->table_cap * 4));
        trace(R, "table_rebuild back");
        TRY(state_pull(c));
        R.i = h->iter - R.rec_base;  // resume after the last recorded merge
        unsample_from(R);
        return 0;
    }
    if (h->halt == HALT_COMM) {
        // what this rank's receive area holds: the exchange it waited for last, and the flags of both halves per sender
        std::string seen;
        if (c->p2p && c->p2p_area) {
            std::vector<unsigned long long> fl(2 * (size_t)c->n_ranks);
            if (hipMemcpy(fl.data(), c->p2p_area + c->p2p_flags_off, fl.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
                for (size_t q = 0; q < fl.size(); ++q) seen += (q ? " " : "") + std::to_string(fl[q]);
            else
                (void)hipGetLastError();
        }
        return fail(c, YABPE_E_COMM, "a peer's records did not arrive within the time limit (peer-to-peer exchange) after %u merges; rank %d launched exchange %llu, "
                    "flags in its receive area [half][sender]: %s", h->iter - R.rec_base, c->rank, (unsigned long long)c->p2p_seq, seen.c_str());
    }
    if (h->halt) {
        const char *why = h->halt == HALT_POOL_FULL ? "token byte pool exhausted (option pool_bytes)"
                          : h->halt == HALT_VOCAB_FULL ? "u16 token id space exhausted"
                                                       : "device halt";
        return fail(c, YABPE_E_CAPACITY, "%s after %u merges", why, h->iter - R.rec_base);
    }
    *next = (h->done || (R.i >= R.num_merges && !c->pending)) ? ROUND_STOP : ROUND_NEXT;
    return 0;
}

// between rounds: the table's load and the stream's fill (the same decisions on every rank)
int round_housekeeping(TrainRun &R) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    if (table_grow_rule(h->table_entries, c->table_cap, R.O.table_load_pct)) {
        trace(R, "table_grow");
        TRY(table_grow(c, table_grow_target_rule(h->table_entries, R.O.table_grow_x, 1ull << 16)));
        trace(R, "table_grow back");
    }
    if (!c->weighted && retile_rule(c->n_tiles, R.O.retile_min_tiles, h->live_slots, R.O.retile_pct, SPAN)) {
        trace(R, "retile");
        TRY(retile_flat(c));
    }
    return 0;
}

// ---- the end of a call
// stops the clock, closes the log of the last iteration (the remaining sites folded into T_i), hands the merges out
int train_close(TrainRun &R, uint32_t *out_left, uint32_t *out_right, uint32_t *out_merged, uint64_t *out_count, uint32_t *out_n_merges) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    HIPCHK(c, hipEventRecord(R.ev.e[1], c->stream));
    HIPCHK(c, hipEventSynchronize(R.ev.e[1]));
    TRY(state_pull(c));
    const uint32_t n = h->iter - R.rec_base;
    TRY(train_copy_out(c, n, true, out_left, out_right, out_merged, out_count, out_n_merges));
    if (n) c->log_sites[n - 1] += h->sites;  // (already closed by the selection when the last launch was a fused one: then h->sites is 0)
    uint64_t sites_all = 0;
    for (uint32_t k = 0; k < n; ++k) sites_all += c->log_sites[k];
    R.tokens_at_start = h->tokens_now - h->sites + sites_all;
    h->tokens_now -= h->sites;
    h->sites = 0;
    TRY(state_push(c));
    return 0;
}

// everything that only feeds yabpe_stats_t: the phases' times, the algorithmic (A_i = 2 * (T_i + W)) and
// actual byte sums, the sampled launches
int train_account(TrainRun &R) {
    yabpe_ctx *c = R.c;
    DevState *h = R.h;
    const uint32_t n = c->rec_n;
    const hipEvent_t t0 = R.ev.e[0], t1 = R.ev.e[1];
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    if (R.split_marked) {
        float sms = 0;
        HIPCHK(c, hipEventElapsedTime(&sms, R.ev.e[2], t1));
        c->stats.sparse_ms += sms;
        c->stats.sparse_merges += n > R.split_at ? n - R.split_at : 0;
        c->stats.sparse_launches += R.launches_sparse;
    }
    if (R.tail_marked) {
        float tms = 0;
        HIPCHK(c, hipEventElapsedTime(&tms, R.ev.e[3], t1));
        c->stats.tail_ms += tms;
        c->stats.tail_merges += n > R.tail_at ? n - R.tail_at : 0;
        c->stats.tail_launches += R.launches_sparse - R.launches_at_tail;
    }
    c->stats.train_ms += ms;
    uint64_t T_ = R.tokens_at_start;
    std::vector<uint64_t> Ti(n);
    for (uint32_t k = 0; k < n; ++k) {
        Ti[k] = T_;
        c->stats.algo_bytes_total += 2 * (T_ + c->n_words_input);
        T_ -= c->log_sites[k];
    }
    // the streaming phase as a whole: its launches, the merges they applied, their algorithmic bytes; a launch applies a batch,
    // so the event-timed launches get the phase's bytes per launch (merge indices of sampled launches are lower bounds)
    uint32_t dense_applied = R.dense_applied;
    uint64_t launches_dense = R.launches_dense;
    if (!R.split_marked) {
        dense_applied = n - std::min<uint32_t>(n, (c->pending && !h->done) ? h->n_batch : 0u);
        launches_dense = h->n_select - std::min<uint32_t>(h->n_select, (c->pending && !h->done) ? 1u : 0u);
    }
    dense_applied = std::min(dense_applied, n);
    uint64_t dense_algo = 0, dense_actual = 0, dense_sampled_now = 0;
    for (uint32_t k = 0; k < dense_applied; ++k) {
        dense_algo += 2 * (Ti[k] + c->n_words_input);
        dense_actual += 2 * c->log_live[k] + 4ull * c->n_tiles;
    }
    // (actual: a pass reads the stream once for all the merges of its batch -- the first merge's live slots)
    c->stats.dense_launches += launches_dense;
    c->stats.dense_merges += dense_applied;
    for (size_t e = 0; e < R.ev_next; ++e) {
        const EventPair &E = c->events[e];
        const uint32_t k = E.iter_rel;
        if (k >= n) continue;
        float ems = 0, sms = 0;
        if (hipEventElapsedTime(&ems, E.e0, E.e2) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (hipEventElapsedTime(&sms, E.e0, E.e1) != hipSuccess) { (void)hipGetLastError(); continue; }
        c->stats.apply_ms_sampled += ems;
        c->ev_iter.push_back(k);
        c->ev_us.push_back(ems * 1000.0f);
        c->ev_scan_us.push_back(sms * 1000.0f);
        c->stats.apply_launches_sampled += 1;
        // streaming form: one pass over the live stream + rewrite (+ selection when fused), a batch of merges.  (A launch queued
        // behind a stop flag -- the rest of a round after a rescan request -- returns in microseconds: not a pass.)
        if (!E.split && ems >= 0.02f) {
            c->stats.dense_ms_sampled += ems;
            dense_sampled_now += 1;
        }
        if (E.split) {  // (sparse form: the merge index of a sampled launch is a lower bound -- launches select batches)
            c->stats.scan_ms_sampled += sms;
            c->stats.scan_launches_sampled += 1;
            c->stats.scan_algo_bytes_sampled += 2 * (Ti[k] + c->n_words_input);
            c->stats.scan_actual_bytes_sampled += 2 * c->log_live[k] + 4ull * c->n_tiles;
        }
        c->stats.apply_algo_bytes_sampled += 2 * (Ti[k] + c->n_words_input);
        c->stats.apply_actual_bytes_sampled += 2 * c->log_live[k] + 4ull * c->n_tiles;
    }
    if (launches_dense && dense_sampled_now) {
        c->stats.dense_launches_sampled += dense_sampled_now;
        c->stats.dense_algo_bytes_sampled += dense_algo * dense_sampled_now / launches_dense;
        c->stats.dense_actual_bytes_sampled += dense_applied ? dense_actual / dense_applied * dense_sampled_now : 0;  // (one read of the live stream per launch)
    }
    return 0;
}
}  // namespace
}  // extern "C++"

int yabpe_train(yabpe_ctx *c, uint32_t num_merges, uint64_t min_frequency, uint32_t *out_left, uint32_t *out_right,
                uint32_t *out_merged, uint64_t *out_count, uint32_t *out_n_merges) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_words) return fail(c, YABPE_E_INVALID, "call yabpe_load_words first");
    if (out_n_merges) *out_n_merges = 0;
    if (c->id_bits == 32) return id32_train(c, num_merges, min_frequency, out_left, out_right, out_merged, out_count, out_n_merges);
    // The u16 id space bounds the vocabulary at YB_MAX_TOKENS; the reference has no such bound (trainer.py:238, 298-300).  A
    // merge that re-creates the bytes of an existing token takes no id (trainer.py:298), so the number of merges a job can run
    // is not bounded by the ids that are left: the request stands as it is, and only when the loop needs an id past the last
    // one does the selection stop it (HALT_VOCAB_FULL -> YABPE_E_CAPACITY in round_recover) -- reported, never silently
    // truncated.  Most such jobs end long before (no pairs left, min_frequency); the per-merge records grow as the loop proceeds.
    TrainRun R{};
    R.c = c;
    R.h = c->st_host;
    R.num_merges = num_merges;
    TRY(train_begin(c, num_merges, min_frequency, &R.rec_base));
    c->kmax_now = 1;
    c->split_mode = false;
    c->sig_valid = false;
    if (num_merges == 0) return YABPE_OK;
    TRY(train_begin_records(c, rec_first_rule(num_merges)));
    R.O = train_opts(c);
    if (R.ev.create() != hipSuccess) return fail(c, YABPE_E_HIP, "event creation failed");
    HIPCHK(c, hipEventRecord(R.ev.e[0], c->stream));
    c->use_cand = false;
    c->pending = false;
    for (RoundNext next = ROUND_NEXT; next != ROUND_STOP;) {
        TRY(round_prepare(R));
        TRY(round_launch(R));
        TRY(round_read(R));
        TRY(round_recover(R, &next));
        if (next == ROUND_NEXT) TRY(round_housekeeping(R));
    }
    TRY(train_close(R, out_left, out_right, out_merged, out_count, out_n_merges));
    TRY(train_account(R));
    if (optv(c, "verify", 0)) {
        uint64_t mm = 0;
        TRY(yabpe_verify_table(c, &mm));
        if (mm) return fail(c, YABPE_E_INTERNAL, "incremental pair table differs from a recount in %llu keys", (unsigned long long)mm);
    }
    return YABPE_OK;
}

int yabpe_n_tokens(yabpe_ctx *c, uint32_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(state_pull(c));
    *out = c->st_host->n_tokens;
    return YABPE_OK;
}

int yabpe_token_bytes(yabpe_ctx *c, uint32_t id, uint8_t *out, uint32_t cap, uint32_t *out_len) {
    if (!c || !out_len) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(state_pull(c));
    if (id >= c->st_host->n_tokens) return fail(c, YABPE_E_INVALID, "token id %u out of range", id);
    uint32_t off = 0, len = 0;
    HIPCHK(c, hipMemcpy(&off, c->tt.off + id, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&len, c->tt.len + id, 4, hipMemcpyDeviceToHost));
    *out_len = len;
    if (out && cap >= len && len) HIPCHK(c, hipMemcpy(out, c->tt.pool + off, len, hipMemcpyDeviceToHost));
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- stats / debug
int yabpe_stats(yabpe_ctx *c, yabpe_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(state_pull(c));
    c->stats.n_words = c->n_words;
    c->stats.n_words_input = c->n_words_input;
    c->stats.n_long_words = c->n_long;
    c->stats.tokens_initial = c->tokens_initial;
    c->stats.tokens_now = c->st_host->tokens_now;
    c->stats.merges_done = c->st_host->iter;
    c->stats.n_tiles = c->n_tiles;
    c->stats.live_slots = c->st_host->live_slots;
    c->stats.table_capacity = c->table_cap;
    c->stats.table_entries = c->st_host->table_entries;
    c->stats.cand_rebuilds = c->cand_rebuilds;
    c->stats.cand_rescans = c->cand_rescans;
    c->stats.fused_launches = c->fused_launches;
    c->stats.exchanges = c->exchanges;
    c->stats.exchange_bytes = (c->multi && c->exchanges) ? (16 + (c->xeff_sum / c->exchanges) * sizeof(DeltaRec)) * (uint64_t)c->n_ranks : 0;  // (mean over the exchanges)
    c->stats.exchange_cap_records = c->xcap;
    c->stats.exchange_p2p = c->p2p ? 1 : 0;
    c->stats.exchange_growths = c->exchange_growths;
    c->stats.exchange_max_records = c->exchange_max_records;
    c->stats.scan_skip_launches = c->scan_skip_launches;
    c->stats.scan_skip_tiles_read = 0;
    c->stats.scan_skip_pieces_taken = 0;
    c->stats.pool_growths = c->pool_growths32;
    if (c->blk_read) {
        std::vector<unsigned long long> br(2 * MAX_LISTS);
        HIPCHK(c, hipMemcpy(br.data(), c->blk_read, 2 * MAX_LISTS * 8, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < MAX_LISTS; ++i) c->stats.scan_skip_tiles_read += br[i];
        for (uint32_t i = MAX_LISTS; i < 2 * MAX_LISTS; ++i) c->stats.scan_skip_pieces_taken += br[i];
    }
    *out = c->stats;
    return YABPE_OK;
}

int yabpe_latency_probe(yabpe_ctx *c, yabpe_latency_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    // 2 GiB of u32 (eight times the Infinity Cache: a hop finds its line in no cache); 512 MiB when the device is nearly full
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint32_t n = free_b > (8ull << 30) ? (1u << 29) : (1u << 27);
    uint32_t *next = nullptr, *sink = nullptr;
    unsigned long long *ticks = nullptr;
    struct Guard {  // (every way out frees the probe's buffers)
        uint32_t *&a, *&b;
        unsigned long long *&t;
        ~Guard() { dfree(a); dfree(b); dfree(t); }
    } guard{next, sink, ticks};
    TRY(dmalloc(c, &next, n));
    TRY(dmalloc(c, &sink, 1));
    TRY(dmalloc(c, &ticks, 1));
    double trip[3] = {0, 0, 0};
    const uint32_t hops = 1024;
    for (int mode = 0; mode < 3; ++mode) {
        // (the table is rewritten before every walk: whatever the last walk left in the caches is pushed out, and each walk is timed once, cold)
        hipLaunchKernelGGL(k_chain_init, dim3(n / 256), dim3(256), 0, c->stream, next, n, (uint32_t)mode);  // (one cycle over all entries, no fixed stride)
        hipLaunchKernelGGL(k_chain_walk, dim3(1), dim3(1), 0, c->stream, next, hops, mode, ticks, sink);
        HIPCHK(c, hipGetLastError());
        unsigned long long t = 0;
        HIPCHK(c, hipMemcpyAsync(&t, ticks, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        trip[mode] = (double)t / 100.0 / hops;
    }
    // dependent empty launches back to back
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    double gap = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        const int n_launch = 400;
        for (int k = 0; k < 50; ++k) hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, c->stream, sink);
        HIPCHK(c, hipEventRecord(e0, c->stream));
        for (int k = 0; k < n_launch; ++k) hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, c->stream, sink);
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        gap = std::min(gap, (double)ms * 1000.0 / n_launch);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    out->launch_gap_us = gap;
    out->load_trip_us = trip[0];
    out->coherent_trip_us = trip[1];
    out->atomic_trip_us = trip[2];
    return YABPE_OK;
}

int yabpe_iter_log(yabpe_ctx *c, uint64_t *out_sites, uint64_t *out_live_slots, uint32_t cap, uint32_t *out_n) {
    if (!c || !out_n) return YABPE_E_INVALID;
    uint32_t n = std::min<uint32_t>(cap, (uint32_t)c->log_sites.size());
    if (out_sites) memcpy(out_sites, c->log_sites.data(), (size_t)n * 8);
    if (out_live_slots) memcpy(out_live_slots, c->log_live.data(), (size_t)n * 8);
    *out_n = (uint32_t)c->log_sites.size();
    return YABPE_OK;
}

int yabpe_event_log(yabpe_ctx *c, uint32_t *out_iter, float *out_us, float *out_scan_us, uint32_t cap, uint32_t *out_n) {
    if (!c || !out_n) return YABPE_E_INVALID;
    uint32_t n = std::min<uint32_t>(cap, (uint32_t)c->ev_iter.size());
    if (out_iter) memcpy(out_iter, c->ev_iter.data(), (size_t)n * 4);
    if (out_us) memcpy(out_us, c->ev_us.data(), (size_t)n * 4);
    if (out_scan_us) memcpy(out_scan_us, c->ev_scan_us.data(), (size_t)n * 4);
    *out_n = (uint32_t)c->ev_iter.size();
    return YABPE_OK;
}

int yabpe_verify_table(yabpe_ctx *c, uint64_t *out_mismatches) {
    if (!c || !out_mismatches) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_words) return fail(c, YABPE_E_INVALID, "no corpus loaded");
    if (c->id_bits == 32) return id32_verify(c, out_mismatches);
    PairTable scratch{};
    HIPCHK(c, hipMemsetAsync(&c->scratch64[4], 0, 16, c->stream));  // [4] entries, [5] mismatches
    TRY(table_alloc(c, scratch, c->table_cap, &c->scratch64[4]));
    TRY(launch_count(c, scratch));
    uint32_t grid = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, c->table_cap / BLOCK));
    const bool dbg = getenv("YABPE_DEBUG_VERIFY") != nullptr;
    unsigned long long *dump = nullptr;
    if (dbg) {
        TRY(dmalloc(c, &dump, 48));
        HIPCHK(c, hipMemsetAsync(dump, 0, 48 * 8, c->stream));
    }
    CmpParams A{c->table, scratch, &c->scratch64[5], dump};
    hipLaunchKernelGGL(k_table_compare, dim3(grid), dim3(BLOCK), 0, c->stream, A);
    CmpParams B{scratch, c->table, &c->scratch64[5], dump};
    hipLaunchKernelGGL(k_table_compare, dim3(grid), dim3(BLOCK), 0, c->stream, B);
    HIPCHK(c, hipGetLastError());
    unsigned long long mm = 0;
    HIPCHK(c, hipMemcpyAsync(&mm, &c->scratch64[5], 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dbg) {
        unsigned long long d[48];
        HIPCHK(c, hipMemcpy(d, dump, sizeof d, hipMemcpyDeviceToHost));
        for (unsigned i = 0; i < 16 && i < mm; ++i)
            fprintf(stderr, "[yabpe verify r%d] key (%llu,%llu) first %lld second %lld\n", c->rank, d[3 * i] >> 16, d[3 * i] & 0xffffull, (long long)d[3 * i + 1], (long long)d[3 * i + 2]);
        dfree(dump);
    }
    table_free(scratch);
    // the recount may have raised halt_req on the scratch table; it is not a training halt
    HIPCHK(c, hipMemsetAsync(&c->st->halt_req, 0, 4, c->stream));
    *out_mismatches = mm;
    return YABPE_OK;
}

int yabpe_stream_checksum(yabpe_ctx *c, uint64_t *out_sum, uint64_t *out_words, uint64_t *out_tokens) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_words) return fail(c, YABPE_E_INVALID, "no corpus loaded");
    if (c->id_bits == 32) return fail(c, YABPE_E_INVALID, "yabpe_stream_checksum reads the u16 stream: not available with id_bits = 32");
    HIPCHK(c, hipMemsetAsync(&c->scratch64[4], 0, 24, c->stream));
    if (c->n_tiles) {
        ChecksumParams P{c->tiles, c->tile_len, c->tile_wbase, c->wfreq, c->n_tiles, c->tt,
                         &c->scratch64[4], &c->scratch64[5], &c->scratch64[6]};
        hipLaunchKernelGGL(k_stream_checksum, dim3(cdiv64(c->n_tiles, BLOCK)), dim3(BLOCK), 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
    }
    if (c->n_long) {  // the words outside the tile stream
        LongChecksumParams L{c->long_tok, c->long_off, c->long_len, c->long_freq, c->n_long, c->tt, &c->scratch64[4], &c->scratch64[5], &c->scratch64[6]};
        hipLaunchKernelGGL(k_long_checksum, dim3(cdiv64(c->n_long, BLOCK)), dim3(BLOCK), 0, c->stream, L);
        HIPCHK(c, hipGetLastError());
    }
    unsigned long long r[3];
    HIPCHK(c, hipMemcpyAsync(r, &c->scratch64[4], 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (out_sum) *out_sum = r[0];
    if (out_words) *out_words = r[1];
    if (out_tokens) *out_tokens = r[2];
    return YABPE_OK;
}

int yabpe_stream_dump(yabpe_ctx *c, uint32_t *out_n_tiles, uint32_t *out_flags, uint16_t *tiles, uint32_t *tile_len, uint32_t *tile_wbase,
                      uint64_t *sig) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->id_bits == 32) return fail(c, YABPE_E_INVALID, "yabpe_stream_dump hands out u16 slots: not available with id_bits = 32");
    if (!c->have_words) return fail(c, YABPE_E_INVALID, "no corpus loaded");
    const bool has_sig = c->sig_valid && c->sig != nullptr && c->sig_stride >= c->n_tiles;
    if (out_n_tiles) *out_n_tiles = c->n_tiles;
    if (out_flags) *out_flags = (c->tile_wbase ? YABPE_DUMP_WBASE : 0u) | (has_sig ? YABPE_DUMP_SIG : 0u);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->n_tiles == 0) return YABPE_OK;
    const size_t n = c->n_tiles;
    if (tiles) HIPCHK(c, hipMemcpy(tiles, c->tiles, n * CAP * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (tile_len) HIPCHK(c, hipMemcpy(tile_len, c->tile_len, n * 4, hipMemcpyDeviceToHost));
    if (tile_wbase && c->tile_wbase) HIPCHK(c, hipMemcpy(tile_wbase, c->tile_wbase, n * 4, hipMemcpyDeviceToHost));
    if (sig && has_sig)  // (the rows without the padding of their stride)
        HIPCHK(c, hipMemcpy2D(sig, n * 8, c->sig, (size_t)c->sig_stride * 8, n * 8, SIG_ROWS, hipMemcpyDeviceToHost));
    return YABPE_OK;
}

int yabpe_memcpy_d2h(yabpe_ctx *c, void *dst_host, const void *src_dev, uint64_t n) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst_host, src_dev, n, hipMemcpyDeviceToHost));
    return YABPE_OK;
}

#ifdef YB_PROFILE_SCAN
int yabpe_debug_sel_profile(unsigned long long out[16]) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_sel_prof), 128) == hipSuccess ? 0 : -1;
}
int yabpe_debug_sel_acc(unsigned long long out[72]) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_sel_acc), 72 * 8) == hipSuccess ? 0 : -1;
}
int yabpe_debug_ss_profile(unsigned long long out[8]) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_ss_prof), 64) == hipSuccess ? 0 : -1;
}
int yabpe_debug_launch_profile(unsigned long long *out, int reset) { // 65536 x 4 u64
    if (reset) {
        std::vector<unsigned long long> z(65536 * 4, 0ull);
        for (size_t i = 0; i < 65536; ++i) z[i * 4] = ~0ull;
#ifdef YB_PROFILE_LAUNCH
        {
            std::vector<unsigned long long> zw(65536 * 8, 0ull);
            if (hipMemcpyToSymbol(HIP_SYMBOL(yb::g_launch_wg), zw.data(), zw.size() * 8) != hipSuccess) return -1;
        }
#endif
        return hipMemcpyToSymbol(HIP_SYMBOL(yb::g_launch_prof), z.data(), z.size() * 8) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_launch_prof), (size_t)65536 * 32) == hipSuccess ? 0 : -1;
}
#ifdef YB_PROFILE_LAUNCH
int yabpe_debug_launch_wg(unsigned long long *out) { // 65536 x 8 u64
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_launch_wg), (size_t)65536 * 64) == hipSuccess ? 0 : -1;
}
#endif
int yabpe_debug_stop_hist(unsigned long long *out) { // 65536 x u64
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_stop_hist), (size_t)65536 * 8) == hipSuccess ? 0 : -1;
}
int yabpe_debug_scan_profile(unsigned long long *out, uint32_t n_blocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_scan_prof), (size_t)std::min<uint32_t>(n_blocks, yb::MAX_LISTS_PROF) * 64) == hipSuccess ? 0 : -1;
}
int yabpe_debug_flush_profile(unsigned long long *out, uint32_t n_blocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_flush_prof), (size_t)std::min<uint32_t>(n_blocks, yb::FLUSH_PROF_BLOCKS) * 32) == hipSuccess ? 0 : -1;
}
#endif
#ifdef YB_PROFILE_SLOW
int yabpe_debug_slow_profile(unsigned long long out[8]) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yb::g_slow_prof), 64) == hipSuccess ? 0 : -1;
}
#endif

int yabpe_memcpy_h2d(yabpe_ctx *c, void *dst_dev, const void *src_host, uint64_t n) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst_dev, src_host, n, hipMemcpyHostToDevice));
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- synthetic corpus
int yabpe_synth_generate(yabpe_ctx *c, uint64_t target_bytes, uint32_t n_types, uint64_t seed, const uint8_t *alphabet,
                         uint32_t alphabet_len, int space_prefix, uint8_t **out_dev_bytes, uint64_t **out_dev_off,
                         uint64_t *out_n_words, uint64_t *out_n_bytes) {
    if (!c || !alphabet || !alphabet_len || !n_types || !out_dev_bytes || !out_dev_off || !out_n_words || !out_n_bytes)
        return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    SynthOut so{};
    int r = synth_generate(c->stream, target_bytes, n_types, seed, alphabet, alphabet_len, space_prefix, &so);
    if (r != 0) return fail(c, r == -2 ? YABPE_E_INTERNAL : YABPE_E_HIP, "synthetic generation failed (%d): %s", r, hipGetErrorString(hipGetLastError()));
    c->synth_bufs.push_back(so.bytes);
    c->synth_bufs.push_back(so.off);
    *out_dev_bytes = so.bytes;
    *out_dev_off = (uint64_t *)so.off;
    *out_n_words = so.n_words;
    *out_n_bytes = so.n_bytes;
    return YABPE_OK;
}

int yabpe_synth_generate_lex(yabpe_ctx *c, uint64_t target_bytes, uint32_t n_types, uint64_t seed, const uint8_t *lex_bytes,
                             const uint64_t *lex_off, uint8_t **out_dev_bytes, uint64_t **out_dev_off, uint64_t *out_n_pieces, uint64_t *out_n_bytes) {
    if (!c || !lex_bytes || !lex_off || !n_types || !out_dev_bytes || !out_dev_off || !out_n_pieces || !out_n_bytes) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    for (uint32_t j = 0; j < n_types; ++j)
        if (lex_off[j + 1] <= lex_off[j] || lex_off[j + 1] - lex_off[j] > 0xFFFFu) return fail(c, YABPE_E_INVALID, "lexicon entry %u is empty or longer than 65,535 bytes", j);
    // expected bytes per draw under the Zipf weights: how many draws the target needs (more if that falls short)
    long double num = 0, den = 0;
    for (uint32_t j = 0; j < n_types; ++j) {
        const long double w = (long double)((1ull << 40) / (j + 1ull));
        num += w * (long double)(lex_off[j + 1] - lex_off[j]);
        den += w;
    }
    const double mean_len = (double)(num / den);
    SynthOut so{};
    int r = -2;
    for (double slack = 1.02; r == -2 && slack < 3.0; slack *= 1.25)
        r = synth_generate_lex(c->stream, target_bytes, n_types, seed, lex_bytes, (const unsigned long long *)lex_off,
                               (unsigned long long)((double)target_bytes / mean_len * slack) + 65536, &so);
    if (r != 0) return fail(c, r == -2 ? YABPE_E_INTERNAL : YABPE_E_HIP, "synthetic text generation failed (%d): %s", r, hipGetErrorString(hipGetLastError()));
    c->synth_bufs.push_back(so.bytes);
    c->synth_bufs.push_back(so.off);
    *out_dev_bytes = so.bytes;
    *out_dev_off = (uint64_t *)so.off;
    *out_n_pieces = so.n_words;
    *out_n_bytes = so.n_bytes;
    return YABPE_OK;
}

int yabpe_synth_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    free_bufs(c->synth_bufs);
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- pre-tokeniser
int yabpe_pretokenize(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off, uint32_t n_chunks,
                      const uint8_t *special_bytes, const uint32_t *special_off, uint32_t n_special,
                      const uint8_t **out_dev_text, uint64_t **out_dev_word_off, uint64_t *out_n_words, int64_t *out_bad_pos) {
    if (!c || !out_dev_text || !out_dev_word_off || !out_n_words || !out_bad_pos) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_text = nullptr; *out_dev_word_off = nullptr; *out_n_words = 0; *out_bad_pos = -1;
    if (n_bytes && !text) return fail(c, YABPE_E_INVALID, "text is NULL");
    if (n_special > 255) return fail(c, YABPE_E_CAPACITY, "at most 255 special tokens in the pre-tokeniser");
    if (n_special && (!special_bytes || !special_off)) return fail(c, YABPE_E_INVALID, "special token arrays are NULL");
    uint32_t max_len = 0;
    for (uint32_t s = 0; s < n_special; ++s) {
        if (special_off[s + 1] <= special_off[s])
            return fail(c, YABPE_E_INVALID, "special token %u is empty (it would match at every position)", s);
        max_len = std::max(max_len, special_off[s + 1] - special_off[s]);
    }
    uint32_t G = 0, pattern = 0;
    TRY(digit_group_opt(c, &G));
    TRY(split_pattern_opt(c, G, &pattern));
    for (uint32_t s = 0; G && s < n_special; ++s) { // group_logic.h: such a special could match where no GPT-2 token starts
        const uint8_t *b = special_bytes + special_off[s];
        const uint64_t len = special_off[s + 1] - special_off[s];
        const PtView v{b, nullptr, len, 0};
        uint32_t cp = 0;
        if (pt_decode(v, 0, len, &cp) && class_of(cp) == PT_N)
            return fail(c, YABPE_E_INVALID, "special token %u (\"%.*s\") begins with a \\p{N} character: not allowed with digit_group = %u", s,
                        (int)std::min<uint64_t>(len, 64), (const char *)b, G);
        // split4_logic.h: whether a token starts at a whitespace character can be open until the scan pass has run
        if (pattern && pt_decode(v, 0, len, &cp) && class_of(cp) == PT_S)
            return fail(c, YABPE_E_INVALID, "special token %u (\"%.*s\") begins with a \\s character: not allowed with split_pattern = %u", s,
                        (int)std::min<uint64_t>(len, 64), (const char *)b, pattern);
    }
    if (pattern == 3 && n_special) { // split5_logic.h: occurrences must never overlap
        uint32_t a = 0, b = 0;
        const int why = s5_specials_check(special_bytes, special_off, n_special, &a, &b);
        const int la = (int)std::min<uint32_t>(special_off[a + 1] - special_off[a], 64), lb = (int)std::min<uint32_t>(special_off[b + 1] - special_off[b], 64);
        const char *sa = (const char *)special_bytes + special_off[a], *sb = (const char *)special_bytes + special_off[b];
        if (why == 1)
            return fail(c, YABPE_E_INVALID, "special token %u (\"%.*s\") contains special token %u (\"%.*s\"): not allowed with split_pattern = 3", a, la, sa, b, lb, sb);
        if (why == 2)
            return fail(c, YABPE_E_INVALID, "an end of special token %u (\"%.*s\") begins special token %u (\"%.*s\"): not allowed with split_pattern = 3", a, la, sa, b, lb, sb);
    }
    std::vector<unsigned long long> chunks;
    TRY(offset_table(c, chunk_off, n_chunks, n_bytes, "chunk", &chunks));
    TRY(class_table(c));
    if (pattern == 3) TRY(class_table5(c));
    // inputs on the device
    Scratch S(c->device, c->rank);
    const uint8_t *d_text = nullptr;
    TRY(to_device(c, S, text, n_bytes, 1, &d_text));
    unsigned long long *d_chunks = nullptr;
    if (S.get(&d_chunks, chunks.size()) != hipSuccess ||
        hipMemcpy(d_chunks, chunks.data(), chunks.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(c, YABPE_E_HIP, "chunk table");
    PtSpecials sp{nullptr, nullptr, n_special, max_len};
    if (n_special) {
        const uint32_t tot = special_off[n_special];
        uint8_t *d_spb = nullptr;
        uint32_t *d_spo = nullptr;
        if (S.get(&d_spb, tot) != hipSuccess || S.get(&d_spo, n_special + 1) != hipSuccess ||
            hipMemcpy(d_spb, special_bytes, tot, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_spo, special_off, (n_special + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(c, YABPE_E_HIP, "special token table");
        sp.bytes = d_spb;
        sp.off = d_spo;
    }
    PretokOut po{};
    if (pretokenize(c->stream, d_text, n_bytes, d_chunks, (uint32_t)chunks.size(), pattern == 3 ? c->pt_cls5 : c->pt_cls, sp, G, pattern, &po) != 0)
        return fail(c, YABPE_E_HIP, "pre-tokeniser failed: %s", hipGetErrorString(hipGetLastError()));
    if (po.bad_pos >= 0) {
        *out_bad_pos = po.bad_pos;
        return fail(c, YABPE_E_UTF8, "invalid UTF-8 at byte %lld", po.bad_pos);
    }
    if (d_text != text) c->pretok_bufs.push_back(S.take(const_cast<uint8_t *>(d_text)));  // (the staged text is handed out)
    c->pretok_bufs.push_back(po.off);
    *out_dev_text = d_text;
    *out_dev_word_off = (uint64_t *)po.off;
    *out_n_words = po.n_words;
    return YABPE_OK;
}

int yabpe_pretokenize_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    free_bufs(c->pretok_bufs);
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- normaliser
// the tables of unicode_norm.inc on the device (the property per code point expanded to 0x110000 entries), built on first use
static int nfc_tables(yabpe_ctx *c, NfcTables *T) {
    if (!c->nfc_prop) {
        if (YB_NFC_PROP_NRUNS < 2 || YB_NFC_PROP_RUNS[0][1] != 0 || YB_NFC_PROP_RUNS[1][0] < NFC_FIRST || YB_NFC_DECOMP[0][0] < NFC_FIRST_DECOMP)
            return fail(c, YABPE_E_INTERNAL, "unicode_norm.inc: a code point below U+%04X has a property", NFC_FIRST);
        std::vector<uint16_t> prop(0x110000, 0);
        for (unsigned r = 0; r < YB_NFC_PROP_NRUNS; ++r) {
            const unsigned lo = YB_NFC_PROP_RUNS[r][0];
            const unsigned hi = r + 1 < YB_NFC_PROP_NRUNS ? YB_NFC_PROP_RUNS[r + 1][0] : 0x110000;
            std::fill(prop.begin() + lo, prop.begin() + hi, (uint16_t)YB_NFC_PROP_RUNS[r][1]);
        }
        uint16_t *d_prop = nullptr;
        uint32_t *d_dec = nullptr, *d_pairs = nullptr;
        Scratch S(c->device, c->rank);
        HIPCHK(c, S.get(&d_prop, prop.size()));
        HIPCHK(c, S.get(&d_dec, (uint64_t)YB_NFC_NDECOMP * 5));
        HIPCHK(c, S.get(&d_pairs, (uint64_t)YB_NFC_NPAIRS * 3));
        HIPCHK(c, hipMemcpy(d_prop, prop.data(), prop.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_dec, YB_NFC_DECOMP, sizeof(YB_NFC_DECOMP), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_pairs, YB_NFC_PAIRS, sizeof(YB_NFC_PAIRS), hipMemcpyHostToDevice));
        c->nfc_prop = S.take(d_prop);
        c->nfc_decomp = S.take(d_dec);
        c->nfc_pairs = S.take(d_pairs);
    }
    *T = NfcTables{c->nfc_prop, c->nfc_decomp, c->nfc_pairs, YB_NFC_NDECOMP, YB_NFC_NPAIRS};
    return 0;
}

int yabpe_normalize_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    free_bufs(c->norm_bufs);
    return YABPE_OK;
}

int yabpe_normalize_stats(yabpe_ctx *c, yabpe_normalize_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->norm_stats;
    return YABPE_OK;
}

// norm_ev[0..1] around the class pass, [1..2] the search for the dirty segments, [2..3] their lengths, [3..4] the write passes
static void normalize_times(yabpe_ctx *c, int last) {
    float ms[4] = {0, 0, 0, 0};
    c->norm_stats.total_ms = pass_times(c->norm_ev, last, ms);
    c->norm_stats.class_ms = ms[0];
    c->norm_stats.find_ms = ms[1];
    c->norm_stats.segments_ms = ms[2];
    c->norm_stats.write_ms = ms[3];
}

int yabpe_normalize(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts, uint32_t form,
                    const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes, int64_t *out_bad_pos) {
    if (!c || !out_dev_text || !out_dev_part_off || !out_n_bytes || !out_bad_pos) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_bad_pos = -1;
    TextPass tp(c, c->norm_bufs, out_dev_text, out_dev_part_off, out_n_bytes);
    if (form != YABPE_NORM_NFC) return fail(c, YABPE_E_INVALID, "normalisation form %u: only YABPE_NORM_NFC (1) is there", form);
    TRY(tp.check(text, n_bytes, part_off, n_parts));
    NfcTables T{};
    TRY(nfc_tables(c, &T));
    TRY(tp.begin(c->norm_stats, c->norm_ev, 1));
    if (tp.n == 0) return tp.hand_out_input();
    Scratch &S = tp.S;
    hipStream_t s = c->stream;
    const uint8_t *d_text = tp.d_text;
    unsigned long long *const d_parts = tp.d_parts;
    const unsigned long long n = tp.n;
    const uint32_t np = tp.np;
    // ---- class: part marks, UTF-8 check, suspects
    uint8_t *marks = nullptr;
    unsigned long long *ctr = nullptr;  // [0] first malformed byte, [1] suspects, [2] first segment over the cap, [3] long segments, [4] bytes copied
    HIPCHK(c, S.get(&marks, n));
    HIPCHK(c, S.get(&ctr, 5));
    const unsigned long long ctr0[5] = {~0ull, 0, ~0ull, 0, 0};
    unsigned long long h_ctr[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipEventRecord(c->norm_ev[0], s));
    HIPCHK(c, hipMemsetAsync(marks, 0, n, s));
    HIPCHK(c, hipMemcpyAsync(ctr, ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pt_mark_chunks, dim3((np + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, marks, (const unsigned long long *)d_parts, np, n);
    const unsigned long long n_pieces = (n + NFC_PIECE - 1) / NFC_PIECE;
    const uint32_t cgrid = (uint32_t)std::min<unsigned long long>((n_pieces + BLOCK - 1) / BLOCK, (unsigned long long)c->n_cu * 16);
    hipLaunchKernelGGL(k_nfc_class, dim3(cgrid), dim3(BLOCK), 0, s, d_text, (const uint8_t *)marks, (uint8_t *)nullptr, n, T, ctr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->norm_ev[1], s));
    HIPCHK(c, hipMemcpyAsync(h_ctr, ctr, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h_ctr[0] != ~0ull) {
        *out_bad_pos = (int64_t)h_ctr[0];
        return fail(c, YABPE_E_UTF8, "invalid UTF-8 at byte %lld", (long long)h_ctr[0]);
    }
    c->norm_stats.n_suspects = h_ctr[1];
    if (h_ctr[1] == 0) {  // the text is NFC
        normalize_times(c, 1);
        return tp.hand_out_input();
    }
    // ---- find: the meta bytes, the segment start of every suspect, the list of dirty segments
    uint8_t *meta = nullptr, *flags = nullptr;
    HIPCHK(c, S.get(&meta, n));
    HIPCHK(c, S.get(&flags, n + 8));
    HIPCHK(c, hipMemsetAsync(flags, 0, n + 8, s));
    HIPCHK(c, hipMemsetAsync(ctr + 1, 0, 8, s));
    hipLaunchKernelGGL(k_nfc_class, dim3(cgrid), dim3(BLOCK), 0, s, d_text, (const uint8_t *)marks, meta, n, T, ctr);
    NfcPos *win = nullptr;
    HIPCHK(c, nfc_find(s, S, meta, flags, n, &win));
    unsigned long long *dstart = nullptr, n_dirty = 0;
    if (pt_offsets(s, S, flags, n, ~0ull, &dstart, &n_dirty) != 0) return fail(c, YABPE_E_HIP, "normaliser: list of dirty segments: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipEventRecord(c->norm_ev[2], s));
    HIPCHK(c, hipStreamSynchronize(s));  // (the scatter still reads the flags; the blocks go back to a cache other streams draw from)
    S.release(flags);
    S.release(win);
    S.release(marks);
    c->norm_stats.n_dirty = n_dirty;
    if (n_dirty == 0) return fail(c, YABPE_E_INTERNAL, "normaliser: %llu suspects and no dirty segment", h_ctr[1]);
    // ---- segments: lengths of the short ones, then of those that need the long path; the scan of out - in
    NfcSegParams P{};
    P.text = d_text; P.meta = meta; P.n = n; P.T = T; P.dstart = dstart; P.n_dirty = n_dirty; P.ctr = ctr + 2;
    unsigned long long *shift = nullptr, *loff = nullptr;
    HIPCHK(c, S.get(&P.dend, n_dirty));
    HIPCHK(c, S.get(&P.delta, n_dirty));
    HIPCHK(c, S.get(&P.nent, n_dirty));
    HIPCHK(c, S.get(&P.long_list, n_dirty));
    HIPCHK(c, S.get(&shift, n_dirty + 1));
    const uint32_t sgrid = (uint32_t)std::min<unsigned long long>((n_dirty + BLOCK - 1) / BLOCK, 1u << 20);
    hipLaunchKernelGGL(k_nfc_short, dim3(sgrid), dim3(BLOCK), 0, s, P, 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_ctr + 2, ctr + 2, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h_ctr[2] != ~0ull) {
        *out_bad_pos = (int64_t)h_ctr[2];
        return fail(c, YABPE_E_CAPACITY, "the segment that starts at byte %lld holds more than %u code points to normalise together (a base and its "
                    "combining marks): over the cap of %u", (long long)h_ctr[2], NFC_CAP, NFC_CAP);
    }
    const unsigned long long n_long = h_ctr[3];
    c->norm_stats.n_dirty_long = n_long;
    uint32_t lgrid = 0;
    if (n_long) {
        HIPCHK(c, S.get(&loff, n_dirty + 1));
        if (exclusive_scan<uint32_t>(s, P.nent, n_dirty, loff, n_dirty + 1) != 0) return fail(c, YABPE_E_HIP, "normaliser: scan of the long segments");
        unsigned long long n_ent = 0;
        HIPCHK(c, hipMemcpyAsync(&n_ent, loff + n_dirty, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, S.get(&P.gbuf, n_ent));
        HIPCHK(c, S.get(&P.gtmp, n_ent));
        P.loff = loff;
        lgrid = (uint32_t)std::min<unsigned long long>((n_long + WPB - 1) / WPB, 1u << 20);
        hipLaunchKernelGGL(k_nfc_long, dim3(lgrid), dim3(BLOCK), 0, s, P, n_long, 0);
        HIPCHK(c, hipGetLastError());
    }
    if (exclusive_scan<unsigned long long>(s, P.delta, n_dirty, shift, n_dirty + 1) != 0) return fail(c, YABPE_E_HIP, "normaliser: scan of the lengths");
    unsigned long long grown = 0;
    HIPCHK(c, hipMemcpyAsync(&grown, shift + n_dirty, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->norm_ev[3], s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long n_out = n + grown;  // (mod 2^64: the segments may have shrunk)
    if (n_out > 3 * n) return fail(c, YABPE_E_INTERNAL, "normaliser: %llu bytes out of %llu", n_out, n);
    // ---- write
    uint8_t *out = nullptr;
    unsigned long long *out_off = nullptr;
    HIPCHK(c, S.get(&out, n_out));
    HIPCHK(c, S.get(&out_off, (uint64_t)np + 1));
    P.shift = shift;
    P.out = out;
    const uint32_t wgrid = (uint32_t)std::min<unsigned long long>((n + NFC_WIN - 1) / NFC_WIN, 1u << 20);
    hipLaunchKernelGGL(k_nfc_copy, dim3(wgrid), dim3(BLOCK), 0, s, d_text, n, (const unsigned long long *)dstart, (const unsigned long long *)P.dend,
                       (const unsigned long long *)shift, n_dirty, out, ctr + 4);
    hipLaunchKernelGGL(k_nfc_short, dim3(sgrid), dim3(BLOCK), 0, s, P, 1);
    if (n_long) hipLaunchKernelGGL(k_nfc_long, dim3(lgrid), dim3(BLOCK), 0, s, P, n_long, 1);
    hipLaunchKernelGGL(k_nfc_offsets, dim3(np / BLOCK + 1), dim3(BLOCK), 0, s, (const unsigned long long *)d_parts, np, n_out,
                       (const unsigned long long *)dstart, (const unsigned long long *)shift, n_dirty, out_off);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->norm_ev[4], s));
    HIPCHK(c, hipMemcpyAsync(h_ctr + 4, ctr + 4, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    normalize_times(c, 4);
    c->norm_stats.n_copied = h_ctr[4];
    return tp.hand_out(out, out_off, n_out);
}

// ---------------------------------------------------------------------------------------------- invalid UTF-8
int yabpe_utf8_repair_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    free_bufs(c->utf8_bufs);
    return YABPE_OK;
}

int yabpe_utf8_repair_stats(yabpe_ctx *c, yabpe_utf8_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->utf8_stats;
    return YABPE_OK;
}

// utf8_ev[0..1] around the check pass, [1..2] the scan and the write pass
static void utf8_times(yabpe_ctx *c, int last) {
    float ms[2] = {0, 0};
    c->utf8_stats.total_ms = pass_times(c->utf8_ev, last, ms);
    c->utf8_stats.check_ms = ms[0];
    c->utf8_stats.write_ms = ms[1];
}

int yabpe_utf8_repair(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts, uint32_t mode,
                      const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes) {
    if (!c || !out_dev_text || !out_dev_part_off || !out_n_bytes) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TextPass tp(c, c->utf8_bufs, out_dev_text, out_dev_part_off, out_n_bytes);
    if (mode != YABPE_UTF8_REPLACE && mode != YABPE_UTF8_IGNORE)
        return fail(c, YABPE_E_INVALID, "utf8 mode %u: YABPE_UTF8_REPLACE (1) or YABPE_UTF8_IGNORE (2)", mode);
    TRY(tp.check(text, n_bytes, part_off, n_parts));
    TRY(tp.begin(c->utf8_stats, c->utf8_ev, 1));
    c->utf8_stats.first_bad_pos = -1;
    if (tp.n == 0) return tp.hand_out_input();
    Scratch &S = tp.S;
    hipStream_t s = c->stream;
    const uint8_t *d_text = tp.d_text;
    unsigned long long *const d_parts = tp.d_parts;
    const unsigned long long n = tp.n;
    const uint32_t np = tp.np;
    // ---- check: the charge of every byte, per tile the output bytes and the subparts
    const unsigned long long nt = (n + U8_TILE - 1) / U8_TILE;
    if (nt > 0x7FFFFFFFull) return fail(c, YABPE_E_CAPACITY, "utf8: %llu bytes are more tiles than one launch takes", n);
    uint32_t *osum = nullptr, *tbad = nullptr;
    unsigned long long *ctr = nullptr;  // [0] first ill-formed byte, [1] subparts
    HIPCHK(c, S.get(&osum, nt));
    HIPCHK(c, S.get(&tbad, nt));
    HIPCHK(c, S.get(&ctr, 2));
    const unsigned long long ctr0[2] = {~0ull, 0};
    unsigned long long h_ctr[2] = {0, 0};
    HIPCHK(c, hipEventRecord(c->utf8_ev[0], s));
    HIPCHK(c, hipMemcpyAsync(ctr, ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    const U8CheckParams C{d_text, n, d_parts, np, mode, osum, tbad, ctr};
    hipLaunchKernelGGL(k_u8_check, dim3((uint32_t)nt), dim3(BLOCK), 0, s, C);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->utf8_ev[1], s));
    HIPCHK(c, hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->utf8_stats.n_subparts = h_ctr[1];
    if (h_ctr[1] == 0) {  // the text is valid UTF-8, part by part
        utf8_times(c, 1);
        return tp.hand_out_input();
    }
    c->utf8_stats.first_bad_pos = (int64_t)h_ctr[0];
    // ---- write: every tile at its base, the part offsets with it
    unsigned long long *rbase = nullptr;
    HIPCHK(c, S.get(&rbase, nt + 1));
    if (exclusive_scan<uint32_t>(s, osum, nt, rbase, nt + 1) != 0) return fail(c, YABPE_E_HIP, "utf8: scan of the tile sums");
    unsigned long long n_out = 0;
    HIPCHK(c, hipMemcpyAsync(&n_out, rbase + nt, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_out > 3 * n) return fail(c, YABPE_E_INTERNAL, "utf8: %llu bytes out of %llu", n_out, n);
    uint8_t *out = nullptr;
    unsigned long long *out_off = nullptr;
    HIPCHK(c, S.get(&out, n_out));
    HIPCHK(c, S.get(&out_off, (uint64_t)np + 1));
    const U8WriteParams W{d_text, n, d_parts, np, mode, rbase, tbad, out, out_off};
    hipLaunchKernelGGL(k_u8_write, dim3((uint32_t)nt), dim3(BLOCK), 0, s, W);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->utf8_ev[2], s));
    HIPCHK(c, hipStreamSynchronize(s));
    utf8_times(c, 2);
    return tp.hand_out(out, out_off, n_out);
}

// ---------------------------------------------------------------------------------------------- lower-casing
// the table of unicode_case.inc on the device (one entry per code point, case_logic.h), built on first use
static int case_tables(yabpe_ctx *c, CaseTables *T) {
    if (!c->case_tab) {
        std::vector<uint32_t> tab(CASE_NCP);
        if (!case_expand(tab.data(), YB_CASE_LOWER, YB_CASE_NLOWER, YB_CASE_TWO, YB_CASE_CASED, YB_CASE_NCASED, YB_CASE_IGNORABLE, YB_CASE_NIGNORABLE))
            return fail(c, YABPE_E_INTERNAL, "unicode_case.inc: the code point that lowers to two, or the sigma, is not what case_logic.h names");
        uint32_t *d_tab = nullptr;
        Scratch S(c->device, c->rank);
        HIPCHK(c, S.get(&d_tab, tab.size()));
        HIPCHK(c, hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        c->case_tab = S.take(d_tab);
    }
    *T = CaseTables{c->case_tab};
    return 0;
}

int yabpe_lowercase_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    free_bufs(c->case_bufs);
    return YABPE_OK;
}

int yabpe_lowercase_stats(yabpe_ctx *c, yabpe_lowercase_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->case_stats;
    return YABPE_OK;
}

// case_ev[0..1] around the check pass, [1..2] the scans, [2..3] the write pass (path 1: [1..2] the write pass)
static void lowercase_times(yabpe_ctx *c, int last) {
    float ms[3] = {0, 0, 0};
    c->case_stats.total_ms = pass_times(c->case_ev, last, ms);
    c->case_stats.check_ms = ms[0];
    c->case_stats.scan_ms = last == 3 ? ms[1] : 0.0;
    c->case_stats.write_ms = last == 3 ? ms[2] : ms[1];
}

int yabpe_lowercase(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *part_off, uint32_t n_parts,
                    const uint8_t **out_dev_text, uint64_t **out_dev_part_off, uint64_t *out_n_bytes, int64_t *out_bad_pos) {
    if (!c || !out_dev_text || !out_dev_part_off || !out_n_bytes || !out_bad_pos) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_bad_pos = -1;
    TextPass tp(c, c->case_bufs, out_dev_text, out_dev_part_off, out_n_bytes);
    TRY(tp.check(text, n_bytes, part_off, n_parts));
    CaseTables T{};
    TRY(case_tables(c, &T));
    TRY(tp.begin(c->case_stats, c->case_ev, 16));
    if (tp.n == 0) return tp.hand_out_input();
    Scratch &S = tp.S;
    hipStream_t s = c->stream;
    const uint8_t *d_text = tp.d_text;
    unsigned long long *const d_parts = tp.d_parts;
    const unsigned long long n = tp.n;
    const uint32_t np = tp.np;
    // ---- check: part marks, UTF-8, what changes, the bytes every window writes
    const unsigned long long n_win = (n + CASE_WIN - 1) / CASE_WIN;
    const dim3 wgrid((uint32_t)std::min<unsigned long long>(n_win, (unsigned long long)c->n_cu * 16));  // (a few atomics per workgroup)
    uint8_t *marks = nullptr;
    uint32_t *wout = nullptr;
    unsigned long long *ctr = nullptr;  // [0] first malformed byte, [1] changing code points, [2] length changers, [3] sigmas, [4] final sigmas
    if (np > 1) {  // (one part: no marks, the kernels know that it starts at byte 0)
        HIPCHK(c, S.get(&marks, n));
    }
    HIPCHK(c, S.get(&wout, n_win));
    HIPCHK(c, S.get(&ctr, 5));
    const unsigned long long ctr0[5] = {~0ull, 0, 0, 0, 0};
    unsigned long long h_ctr[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipEventRecord(c->case_ev[0], s));
    HIPCHK(c, hipMemcpyAsync(ctr, ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    if (marks) {
        HIPCHK(c, hipMemsetAsync(marks, 0, n, s));
        hipLaunchKernelGGL(k_pt_mark_chunks, dim3((np + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, marks, (const unsigned long long *)d_parts, np, n);
    }
    const CaseCheckParams C{d_text, marks, n, T, wout, ctr};
    hipLaunchKernelGGL(k_case_check, wgrid, dim3(BLOCK), 0, s, C);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->case_ev[1], s));
    HIPCHK(c, hipMemcpyAsync(h_ctr, ctr, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h_ctr[0] != ~0ull) {
        *out_bad_pos = (int64_t)h_ctr[0];
        return fail(c, YABPE_E_UTF8, "invalid UTF-8 at byte %lld", (long long)h_ctr[0]);
    }
    c->case_stats.n_changed = h_ctr[1];
    c->case_stats.n_resized = h_ctr[2];
    c->case_stats.n_sigma = h_ctr[3];
    if (h_ctr[1] == 0) {  // the text is lower case
        lowercase_times(c, 1);
        return tp.hand_out_input();
    }
    if (h_ctr[2] == 0 && h_ctr[3] == 0) {  // ---- same size
        uint8_t *out = nullptr;
        HIPCHK(c, S.get(&out, n));
        const unsigned long long n_pieces = (n + CASE_PIECE - 1) / CASE_PIECE;
        const uint32_t grid = (uint32_t)std::min<unsigned long long>((n_pieces + BLOCK - 1) / BLOCK, (unsigned long long)c->n_cu * 16);
        hipLaunchKernelGGL(k_case_same, dim3(grid), dim3(BLOCK), 0, s, d_text, n, T, out);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->case_ev[2], s));
        HIPCHK(c, hipStreamSynchronize(s));
        lowercase_times(c, 2);
        c->case_stats.path = 1;
        c->case_stats.n_copied = n;
        return tp.hand_out(out, d_parts, n);  // (the input's offsets)
    }
    // ---- general: the final sigmas, the base of every window
    uint16_t *fin = nullptr;
    if (h_ctr[3]) {
        HIPCHK(c, S.get(&fin, (n + CASE_PIECE - 1) / CASE_PIECE));
        HIPCHK(c, case_sigma_scans(s, S, d_text, marks, n, T, fin));
    }
    unsigned long long *rbase = nullptr;
    HIPCHK(c, S.get(&rbase, n_win + 1));
    if (exclusive_scan<uint32_t>(s, wout, n_win, rbase, n_win + 1) != 0) return fail(c, YABPE_E_HIP, "lowercase: scan of the window sizes");
    unsigned long long n_out = 0;
    HIPCHK(c, hipMemcpyAsync(&n_out, rbase + n_win, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->case_ev[2], s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_out > n + n / 2 + 1) return fail(c, YABPE_E_INTERNAL, "lowercase: %llu bytes out of %llu", n_out, n);
    // ---- write: every window at its base, the part offsets with it
    uint8_t *out = nullptr;
    unsigned long long *out_off = nullptr;
    HIPCHK(c, S.get(&out, n_out + 16));
    HIPCHK(c, S.get(&out_off, (uint64_t)np + 1));
    const CaseWriteParams W{d_text, n, T, fin, d_parts, np, rbase, out, out_off, ctr + 4};
    hipLaunchKernelGGL(k_case_write, wgrid, dim3(BLOCK), 0, s, W);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->case_ev[3], s));
    HIPCHK(c, hipMemcpyAsync(h_ctr + 4, ctr + 4, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    lowercase_times(c, 3);
    c->case_stats.path = 2;
    c->case_stats.n_final_sigma = h_ctr[4];
    c->case_stats.n_copied = n_out;
    return tp.hand_out(out, out_off, n_out);
}

// ---------------------------------------------------------------------------------------------- word pool
// the empty pool with the capacities the options ask for (first add or get after yabpe_create / yabpe_pool_clear)
static int pool_start(yabpe_ctx *c) {
    if (c->have_pool) return 0;
    const unsigned long long slot_cap = pl_pow2((unsigned long long)std::max<int64_t>(2, std::min<int64_t>(optv(c, "pool_init_slots", 1 << 16), 1ll << 32)));
    const unsigned long long arena_cap = (unsigned long long)std::max<int64_t>(1, optv(c, "pool_init_bytes", 1 << 20));
    Scratch S(c->device, c->rank);
    PoolView V{};
    HIPCHK(c, S.get(&V.arena, arena_cap));
    HIPCHK(c, S.get(&V.off, pl_words_for(slot_cap) + 1));
    HIPCHK(c, S.get(&V.count, pl_words_for(slot_cap)));
    HIPCHK(c, S.get(&V.hash, pl_words_for(slot_cap)));
    HIPCHK(c, S.get(&V.slots, slot_cap));
    V.slot_cap = slot_cap;
    V.hash_bits = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(optv(c, "pool_hash_bits", 64), 64));
    HIPCHK(c, hipMemsetAsync(V.slots, 0xFF, slot_cap * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(V.off, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.take(V.arena); S.take(V.off); S.take(V.count); S.take(V.hash); S.take(V.slots);
    c->wpool = V;
    c->wpool_arena_cap = arena_cap;
    c->wpool_n = c->wpool_bytes = 0;
    c->wpool_stats = yabpe_pool_stats_t{};
    c->have_pool = true;
    return 0;
}

int yabpe_pool_clear(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    if (c->have_pool) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        dfree(c->wpool.arena); dfree(c->wpool.off); dfree(c->wpool.count); dfree(c->wpool.hash); dfree(c->wpool.slots);
    }
    c->wpool = PoolView{};
    c->wpool_arena_cap = c->wpool_n = c->wpool_bytes = 0;
    c->wpool_stats = yabpe_pool_stats_t{};
    c->have_pool = false;
    return YABPE_OK;
}

int yabpe_pool_add(yabpe_ctx *c, const uint8_t *bytes, const uint64_t *word_off, const uint64_t *word_freq, uint64_t n_words) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_words >= PL_MAX_WORDS) return fail(c, YABPE_E_CAPACITY, "2^32-2 words or more in one yabpe_pool_add call");
    TRY(pool_start(c));
    if (n_words == 0) {
        c->wpool_stats.n_calls++;
        return YABPE_OK;
    }
    if (!word_off) return fail(c, YABPE_E_INVALID, "word_off is NULL");
    for (auto &e : c->wpool_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipEvent_t *ev = c->wpool_ev;
    Scratch S(c->device, c->rank);  // staged inputs, the call-local pooling, the probe's results; a grown pool's old arrays

    // ---- inputs on the device (as load_words_impl reads them)
    const unsigned long long *d_off = nullptr, *d_freq = nullptr;
    const uint8_t *d_bytes = bytes;
    uint64_t total_bytes = 0, off_base = 0;
    if (is_device_ptr(word_off)) {
        HIPCHK(c, hipMemcpy(&total_bytes, word_off + n_words, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&off_base, word_off, 8, hipMemcpyDeviceToHost));
    } else {
        off_base = word_off[0];
        total_bytes = word_off[n_words];
    }
    if (total_bytes < off_base) return fail(c, YABPE_E_INVALID, "word offsets must ascend");
    total_bytes -= off_base;
    if (total_bytes && !bytes) return fail(c, YABPE_E_INVALID, "bytes is NULL");
    TRY(to_device(c, S, (const unsigned long long *)word_off, (n_words + 1) * 8, 1, &d_off));
    if (total_bytes) {
        TRY(to_device(c, S, bytes + off_base, total_bytes, 1, &d_bytes));
        d_bytes -= off_base;  // offsets stay absolute
    }
    if (word_freq) TRY(to_device(c, S, (const unsigned long long *)word_freq, n_words * 8, 1, &d_freq));
    HIPCHK(c, hipEventRecord(ev[0], c->stream));

    // ---- 1. the call's words among themselves: every occurrence is touched here and nowhere else
    PoolOut po{};
    if (pool_words(c->stream, S, d_bytes, d_off, d_freq, n_words, &po) != 0)
        return fail(c, YABPE_E_HIP, "pooling of the call's words failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    const unsigned long long n_call = po.n_unique;  // (>= 1)

    // ---- 2. probe: which of the call's unique words the pool has
    uint32_t *d_ulist = nullptr, *d_hit = nullptr, *d_nflag = nullptr, *d_nlen = nullptr;
    unsigned long long *d_nidx = nullptr, *d_noff = nullptr, *d_misc = nullptr;  // d_misc: [0] too-long flag [1] zero-length count
    HIPCHK(c, S.get(&d_ulist, n_call));
    HIPCHK(c, S.get(&d_hit, n_call));
    HIPCHK(c, S.get(&d_nflag, n_call));
    HIPCHK(c, S.get(&d_nlen, n_call));
    HIPCHK(c, S.get(&d_nidx, n_call + 1));
    HIPCHK(c, S.get(&d_noff, n_call + 1));
    HIPCHK(c, S.get(&d_misc, 2));
    HIPCHK(c, hipMemsetAsync(d_misc, 0, 16, c->stream));
    hipLaunchKernelGGL(k_pool_compact, dim3(cdiv64(n_words, 256)), dim3(256), 0, c->stream, po.flag, po.uidx, (unsigned long long)n_words, d_ulist);
    const PoolCall call{d_bytes, d_off, po.hash, po.count, d_ulist, n_call};
    const uint32_t grid = cdiv64(n_call, BLOCK);
    hipLaunchKernelGGL(k_pool_probe, dim3(grid), dim3(BLOCK), 0, c->stream, PoolProbeParams{call, c->wpool, d_hit, d_nflag, d_nlen, (uint32_t *)d_misc});
    HIPCHK(c, hipGetLastError());

    // ---- 3. where the new words go; room for them
    if (exclusive_scan<uint32_t>(c->stream, d_nflag, n_call, d_nidx, n_call + 1) != 0 ||
        exclusive_scan<uint32_t>(c->stream, d_nlen, n_call, d_noff, n_call + 1) != 0)
        return fail(c, YABPE_E_HIP, "scan of the new words failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipEventRecord(ev[2], c->stream));
    unsigned long long n_new = 0, new_bytes = 0, too_long = 0;
    HIPCHK(c, hipMemcpyAsync(&n_new, d_nidx + n_call, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&new_bytes, d_noff + n_call, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&too_long, d_misc, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (too_long) return fail(c, YABPE_E_CAPACITY, "a single word of 2^32 bytes or more");
    const unsigned long long n_total = c->wpool_n + n_new, bytes_total = c->wpool_bytes + new_bytes;
    if (n_total > PL_MAX_WORDS) return fail(c, YABPE_E_CAPACITY, "the pool would hold more than 2^32-2 unique words");
    // (up to here the pool has only been read; every allocation of the growth is made before anything is replaced)
    PoolView V = c->wpool;
    const bool grow_slots = pl_slots_full(n_total, V.slot_cap), grow_arena = bytes_total > c->wpool_arena_cap;
    const unsigned long long arena_cap = pl_grow(c->wpool_arena_cap, bytes_total);
    Scratch G(c->device, c->rank);
    if (grow_slots) {
        V.slot_cap = pl_slots_for(V.slot_cap, n_total);
        HIPCHK(c, G.get(&V.off, pl_words_for(V.slot_cap) + 1));
        HIPCHK(c, G.get(&V.count, pl_words_for(V.slot_cap)));
        HIPCHK(c, G.get(&V.hash, pl_words_for(V.slot_cap)));
        HIPCHK(c, G.get(&V.slots, V.slot_cap));
    }
    if (grow_arena) HIPCHK(c, G.get(&V.arena, arena_cap));
    if (grow_slots) {
        const PoolView &O = c->wpool;
        HIPCHK(c, hipMemcpyAsync(V.off, O.off, (c->wpool_n + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(V.slots, 0xFF, V.slot_cap * 4, c->stream));
        if (c->wpool_n) {
            HIPCHK(c, hipMemcpyAsync(V.count, O.count, c->wpool_n * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(V.hash, O.hash, c->wpool_n * 8, hipMemcpyDeviceToDevice, c->stream));
            hipLaunchKernelGGL(k_pool_rehash, dim3(cdiv64(c->wpool_n, 256)), dim3(256), 0, c->stream, V.hash, (unsigned long long)c->wpool_n, V.slots, V.slot_cap);
            HIPCHK(c, hipGetLastError());
        }
        S.adopt(O.off); S.adopt(O.count); S.adopt(O.hash); S.adopt(O.slots);  // (freed when the call returns, after the synchronise)
        G.take(V.off); G.take(V.count); G.take(V.hash); G.take(V.slots);
        c->wpool_stats.slot_growths++;
    }
    if (grow_arena) {
        if (c->wpool_bytes) HIPCHK(c, hipMemcpyAsync(V.arena, c->wpool.arena, c->wpool_bytes, hipMemcpyDeviceToDevice, c->stream));
        S.adopt(c->wpool.arena);
        G.take(V.arena);
        c->wpool_arena_cap = arena_cap;
        c->wpool_stats.arena_growths++;
    }
    c->wpool = V;

    // ---- 4. append: counts of the found words, bytes / off / count / hash / slot of the new ones
    hipLaunchKernelGGL(k_pool_append, dim3(grid), dim3(BLOCK), 0, c->stream,
                       PoolAppendParams{call, V, d_hit, d_nidx, d_noff, (unsigned long long)c->wpool_n, (unsigned long long)c->wpool_bytes, d_misc + 1});
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[3], c->stream));
    unsigned long long dropped = 0;
    HIPCHK(c, hipMemcpyAsync(&dropped, d_misc + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->wpool_n = n_total;
    c->wpool_bytes = bytes_total;
    yabpe_pool_stats_t &st = c->wpool_stats;
    st.n_calls++;
    st.n_words_added += n_words;
    st.n_empty_dropped += dropped;
    float ms[4] = {0, 0, 0, 0};
    HIPCHK(c, hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    HIPCHK(c, hipEventElapsedTime(&ms[1], ev[1], ev[2]));
    HIPCHK(c, hipEventElapsedTime(&ms[2], ev[2], ev[3]));
    HIPCHK(c, hipEventElapsedTime(&ms[3], ev[0], ev[3]));
    st.pool_ms = ms[0]; st.probe_ms = ms[1]; st.append_ms = ms[2]; st.total_ms = ms[3];
    return YABPE_OK;
}

int yabpe_pool_get(yabpe_ctx *c, const uint8_t **out_dev_bytes, const uint64_t **out_dev_off, const uint64_t **out_dev_freq,
                   uint64_t *out_n_unique, uint64_t *out_n_bytes) {
    if (!c || !out_dev_bytes || !out_dev_off || !out_dev_freq || !out_n_unique || !out_n_bytes) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(pool_start(c));
    *out_dev_bytes = c->wpool.arena;
    *out_dev_off = (const uint64_t *)c->wpool.off;
    *out_dev_freq = (const uint64_t *)c->wpool.count;
    *out_n_unique = c->wpool_n;
    *out_n_bytes = c->wpool_bytes;
    return YABPE_OK;
}

int yabpe_pool_stats(yabpe_ctx *c, yabpe_pool_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->wpool_stats;
    out->n_unique = c->wpool_n;
    out->n_bytes = c->wpool_bytes;
    out->slot_capacity = c->wpool.slot_cap;
    out->arena_capacity = c->wpool_arena_cap;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- encoder
int yabpe_encode_set_model(yabpe_ctx *c, const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab,
                           const uint8_t *merge_bytes, const uint64_t *merge_off, uint32_t n_merges, const uint8_t *special_bytes,
                           const uint32_t *special_off, uint32_t n_special, uint32_t unk_id) {
    if (!c) return YABPE_E_INVALID;
    if ((n_vocab && (!vocab_bytes || !vocab_off || !vocab_ids)) || (n_merges && (!merge_bytes || !merge_off)) ||
        (n_special && (!special_bytes || !special_off)))
        return fail(c, YABPE_E_INVALID, "model arrays are NULL");
    HIPCHK(c, hipSetDevice(c->device));
    EncModelHost m;
    const int r = enc_build_model(vocab_bytes, vocab_off, vocab_ids, n_vocab, merge_bytes, merge_off, n_merges, special_bytes, special_off,
                                  n_special, unk_id, &m);
    if (r == -1) return fail(c, YABPE_E_INVALID, "a special token is empty (it would match at every position)");
    if (r != 0) return fail(c, YABPE_E_CAPACITY, "at most %u special tokens and 2^32 - 2 interned byte strings", ENC_MAX_SPECIALS);
    c->have_enc_model = false;
    dfree(c->enc_keys); dfree(c->enc_vals); dfree(c->enc_out_id);
    dfree(c->enc_sp_bytes); dfree(c->enc_sp_has); dfree(c->enc_sp_off); dfree(c->enc_sp_id);
    c->enc_keys = nullptr; c->enc_vals = nullptr; c->enc_out_id = nullptr;
    c->enc_sp_bytes = nullptr; c->enc_sp_has = nullptr; c->enc_sp_off = nullptr; c->enc_sp_id = nullptr;
    TRY(dmalloc(c, &c->enc_keys, m.keys.size()));
    TRY(dmalloc(c, &c->enc_vals, m.vals.size()));
    TRY(dmalloc(c, &c->enc_out_id, m.out_id.size()));
    HIPCHK(c, hipMemcpy(c->enc_keys, m.keys.data(), m.keys.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->enc_vals, m.vals.data(), m.vals.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->enc_out_id, m.out_id.data(), m.out_id.size() * 4, hipMemcpyHostToDevice));
    c->enc_mask = m.keys.size() - 1;
    c->enc_n_special = n_special;
    c->enc_sp_max_len = 0;
    if (n_special) {
        for (uint32_t s = 0; s < n_special; ++s) c->enc_sp_max_len = std::max(c->enc_sp_max_len, special_off[s + 1] - special_off[s]);
        TRY(dmalloc(c, &c->enc_sp_bytes, special_off[n_special]));
        TRY(dmalloc(c, &c->enc_sp_off, n_special + 1));
        TRY(dmalloc(c, &c->enc_sp_id, n_special));
        TRY(dmalloc(c, &c->enc_sp_has, n_special));
        HIPCHK(c, hipMemcpy(c->enc_sp_bytes, special_bytes, special_off[n_special], hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->enc_sp_off, special_off, (n_special + 1) * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->enc_sp_id, m.sp_id.data(), n_special * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->enc_sp_has, m.sp_has.data(), n_special, hipMemcpyHostToDevice));
    }
    c->have_enc_model = true;
    return YABPE_OK;
}

int yabpe_encode_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    dfree(c->enc_ids);
    dfree(c->enc_doc);
    dfree(c->enc_spans);
    dfree(c->enc_words);
    c->enc_ids = nullptr;
    c->enc_doc = nullptr;
    c->enc_spans = nullptr;
    c->enc_words = nullptr;
    return YABPE_OK;
}

// The phases every encoder shares, on staged inputs (n > 0): the split (document marks, the special split, classes / UTF-8 /
// pre-token starts; events 0 .. 1) and the pre-token offsets (.. event 2).  Malformed UTF-8: YABPE_E_UTF8, *out_bad_pos.
struct EncFront {
    uint8_t *meta = nullptr, *flags = nullptr, *sflag = nullptr;  // (sflag: nullptr without specials)
    unsigned long long *off = nullptr, n_pre = 0;
};

static int encode_front(yabpe_ctx *c, Scratch &S, const uint8_t *d_text, unsigned long long n, const unsigned long long *d_docs, uint32_t n_docs,
                        int64_t *out_bad_pos, EncFront *F) {
    hipStream_t s = c->stream;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>((n + BLOCK - 1) / BLOCK, 1u << 20);
    uint32_t G = 0, pattern = 0;
    TRY(digit_group_opt(c, &G));
    TRY(split_pattern_opt(c, G, &pattern));
    // ---- split: document marks, the special split, classes / UTF-8 / pre-token starts, digit groups
    uint8_t *meta = nullptr, *flags = nullptr, *sflag = nullptr;
    unsigned long long *err = nullptr;
    HIPCHK(c, S.get(&meta, n));
    HIPCHK(c, S.get(&flags, n + 8));
    HIPCHK(c, S.get(&err, 1));
    if (c->enc_n_special) HIPCHK(c, S.get(&sflag, n));
    HIPCHK(c, hipEventRecord(c->enc_ev[0], s));
    HIPCHK(c, hipMemsetAsync(meta, 0, n, s));
    HIPCHK(c, hipMemsetAsync(err, 0xff, 8, s));
    hipLaunchKernelGGL(k_pt_mark_chunks, dim3((n_docs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, meta, d_docs, n_docs, n);
    const PtSpecials sp{c->enc_sp_bytes, c->enc_sp_off, c->enc_n_special, c->enc_sp_max_len};
    if (sflag) {
        HIPCHK(c, hipMemsetAsync(sflag, 0, n, s));
        hipLaunchKernelGGL(k_enc_special, dim3(grid), dim3(BLOCK), 0, s, d_text, meta, n, sp, sflag);
        hipLaunchKernelGGL(k_enc_segments, dim3(grid), dim3(BLOCK), 0, s, sflag, n, meta);
    }
    PretokParams P{d_text, meta, flags, n, c->pt_cls, err, PtSpecials{nullptr, nullptr, 0, 0}, 0};
    const uint32_t wgrid = (uint32_t)std::min<unsigned long long>((n + PT_WIN - 1) / PT_WIN, 1u << 20);
    if (pattern == 3) { // the marks stay where they are; the classes go to an array of their own, which is the meta from here on
        uint8_t *marks = meta;
        TRY(class_table5(c));
        HIPCHK(c, S.get(&meta, n));
        if (pt_split5(s, S, d_text, marks, meta, flags, n, c->pt_cls5, err, P.sp) != 0)
            return fail(c, YABPE_E_HIP, "o200k_base split failed: %s", hipGetErrorString(hipGetLastError()));
    } else if (pattern) hipLaunchKernelGGL(k_pt4_fused, dim3(wgrid), dim3(BLOCK), 0, s, P);
    else hipLaunchKernelGGL(k_pt_fused, dim3(wgrid), dim3(BLOCK), 0, s, P);
    if (sflag) hipLaunchKernelGGL(k_enc_clear, dim3(grid), dim3(BLOCK), 0, s, sflag, n, flags, (uint8_t)(G ? GRP_INSIDE : 0));
    if (pattern == 1 && pt_newlines(s, S, meta, flags, n) != 0) return fail(c, YABPE_E_HIP, "newline rules failed: %s", hipGetErrorString(hipGetLastError()));
    if (G && pt_group(s, S, meta, flags, n, G) != 0) return fail(c, YABPE_E_HIP, "digit groups failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->enc_ev[1], s));
    unsigned long long h_err = 0;
    HIPCHK(c, hipMemcpyAsync(&h_err, err, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h_err != ~0ull) {
        *out_bad_pos = (int64_t)h_err;
        return fail(c, YABPE_E_UTF8, "invalid UTF-8 at byte %llu", h_err);
    }
    // ---- pre-token offsets
    unsigned long long *off = nullptr, n_pre = 0;
    const int pr = pt_offsets(s, S, flags, n, 0xFFFFFFFEull, &off, &n_pre);
    if (pr == -2) return fail(c, YABPE_E_CAPACITY, "%llu pre-tokens in one call: at most 2^32 - 2", n_pre);
    if (pr != 0) return fail(c, YABPE_E_HIP, "pre-token offsets failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipEventRecord(c->enc_ev[2], s));
    F->meta = meta; F->flags = flags; F->sflag = sflag; F->off = off; F->n_pre = n_pre;
    return YABPE_OK;
}

// yabpe_encode (out_dev_spans == nullptr, out_dev_words == nullptr), yabpe_encode_spans and yabpe_encode_words: one body.
static int encode_run(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint32_t span_flags,
                      uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint64_t **out_dev_spans, uint32_t **out_dev_words, uint64_t *out_n_ids,
                      int64_t *out_bad_pos) {
    const bool spans = out_dev_spans != nullptr, chars = spans && (span_flags & YABPE_SPANS_CHARS), words = out_dev_words != nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_ids = nullptr; *out_dev_doc_off = nullptr; *out_n_ids = 0; *out_bad_pos = -1;
    if (spans) *out_dev_spans = nullptr;
    if (words) *out_dev_words = nullptr;
    if (span_flags & ~YABPE_SPANS_CHARS) return fail(c, YABPE_E_INVALID, "unknown flags 0x%x", span_flags);
    if (!c->have_enc_model) return fail(c, YABPE_E_INVALID, "no model: call yabpe_encode_set_model first");
    uint32_t G_checked = 0;
    TRY(digit_group_opt(c, &G_checked)); // (also when there is no text to split)
    uint32_t pattern_checked = 0;
    TRY(split_pattern_opt(c, G_checked, &pattern_checked));
    if (n_bytes && !text) return fail(c, YABPE_E_INVALID, "text is NULL");
    TRY(check_starts(c, doc_off, n_docs, n_bytes, "text"));
    yabpe_encode_free(c);
    c->enc_done = false;
    c->enc_stats = yabpe_encode_stats_t{};
    c->enc_stats.n_bytes = n_bytes;
    c->enc_stats.n_docs = n_docs;
    TRY(class_table(c));
    for (auto &e : c->enc_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    const unsigned long long n = n_bytes;
    Scratch S(c->device, c->rank);
    // inputs on the device (enc_lead reads the text in aligned 16-byte chunks)
    const uint8_t *d_text = nullptr;
    TRY(to_device(c, S, text, n, chars ? 16 : 1, &d_text));
    unsigned long long *d_docs = nullptr;
    HIPCHK(c, S.get(&d_docs, n_docs));
    HIPCHK(c, hipMemcpy(d_docs, doc_off, (size_t)n_docs * 8, hipMemcpyHostToDevice));
    TRY(dmalloc(c, &c->enc_doc, (uint64_t)n_docs + 1));
    unsigned long long *doc_ids = (unsigned long long *)c->enc_doc;
    if (n == 0) { // every document is empty
        HIPCHK(c, hipMemsetAsync(doc_ids, 0, ((size_t)n_docs + 1) * 8, s));
        TRY(dmalloc(c, &c->enc_ids, 1));
        if (spans) {
            TRY(dmalloc(c, &c->enc_spans, 2));
            *out_dev_spans = (uint64_t *)c->enc_spans;
        }
        if (words) {
            TRY(dmalloc(c, &c->enc_words, 1));
            *out_dev_words = c->enc_words;
        }
        HIPCHK(c, hipStreamSynchronize(s));
        c->enc_sums[0] = c->enc_sums[1] = c->enc_sums[2] = c->enc_sums[3] = 0;
        c->enc_done = true;
        *out_dev_ids = c->enc_ids;
        *out_dev_doc_off = (uint64_t *)c->enc_doc;
        return YABPE_OK;
    }
    EncFront F;
    TRY(encode_front(c, S, d_text, n, d_docs, n_docs, out_bad_pos, &F));
    uint8_t *const sflag = F.sflag;
    unsigned long long *const off = F.off;
    const unsigned long long n_pre = F.n_pre;
    // ---- pooling: each pre-token's representative, the list of unique words
    PoolOut pw{};
    if (pool_words(s, S, d_text, off, nullptr, n_pre, &pw) != 0)
        return fail(c, YABPE_E_HIP, "pooling of the pre-tokens failed: %s", hipGetErrorString(hipGetLastError()));
    uint32_t *const rep = pw.rep, *const flag = pw.flag, *const ulen = pw.ulen;
    unsigned long long *const count = pw.count, *const uidx = pw.uidx, *const uoff = pw.uoff;
    const unsigned long long nu = pw.n_unique, ubytes = pw.unique_bytes;
    const uint32_t pgrid = (uint32_t)((n_pre + 255) / 256);
    uint32_t *ulist = nullptr, *llen = nullptr, *uids = nullptr;
    unsigned long long *lbase = nullptr;
    HIPCHK(c, S.get(&ulist, nu));
    HIPCHK(c, S.get(&llen, nu));
    HIPCHK(c, S.get(&lbase, nu + 1));
    HIPCHK(c, S.get(&uids, ubytes));
    uint32_t *upos = nullptr;
    if (spans) HIPCHK(c, S.get(&upos, ubytes));
    hipLaunchKernelGGL(k_enc_compact, dim3(pgrid), dim3(256), 0, s, flag, uidx, off, n_pre, ulist, llen);
    HIPCHK(c, hipGetLastError());
    if (exclusive_scan<uint32_t>(s, llen, nu, lbase, nu + 1) != 0) return fail(c, YABPE_E_HIP, "scan of the long words failed");
    unsigned long long lbytes = 0;
    HIPCHK(c, hipMemcpyAsync(&lbytes, lbase + nu, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->enc_ev[3], s));
    HIPCHK(c, hipStreamSynchronize(s));
    // ---- the merges of every unique word (flag is free again: it becomes the per-word id count)
    uint32_t *ltok = nullptr, *lnxt = nullptr, *lprv = nullptr;
    unsigned long long *lheap = nullptr, *wsums = nullptr;
    HIPCHK(c, S.get(&ltok, lbytes));
    HIPCHK(c, S.get(&lnxt, lbytes));
    HIPCHK(c, S.get(&lprv, lbytes));
    HIPCHK(c, S.get(&lheap, 3 * lbytes));
    HIPCHK(c, S.get(&wsums, 4));
    HIPCHK(c, hipMemsetAsync(wsums, 0, 32, s));
    HIPCHK(c, hipEventRecord(c->enc_ev[4], s));  // (the words phase starts here: the scratch allocation above is host work)
    EncWordsParams W{d_text, off, ulist, nu, uoff, lbase, count, sflag, EncTable{c->enc_keys, c->enc_vals, c->enc_mask}, c->enc_out_id,
                     c->enc_sp_id, c->enc_sp_has, flag, uids, upos, ltok, lnxt, lprv, lheap, wsums};
    const uint32_t wg = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>((nu + WPB - 1) / WPB, (unsigned long long)c->n_cu * 8));
    if (spans)
        hipLaunchKernelGGL(k_enc_words<true>, dim3(wg), dim3(BLOCK), 0, s, W);
    else
        hipLaunchKernelGGL(k_enc_words<false>, dim3(wg), dim3(BLOCK), 0, s, W);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->enc_ev[5], s));
    // ---- emission: per pre-token count -> id offsets -> ids; per-document offsets
    unsigned long long *id_off = nullptr;
    HIPCHK(c, S.get(&id_off, n_pre + 1));
    const unsigned long long n_gran = (n + ENC_GRANULE - 1) / ENC_GRANULE;
    uint8_t *lead_cnt = nullptr;
    unsigned long long *lead_table = nullptr;
    if (chars) {
        HIPCHK(c, S.get(&lead_cnt, n_gran));
        HIPCHK(c, S.get(&lead_table, n_gran + 1));
    }
    HIPCHK(c, hipEventRecord(c->enc_ev[6], s));
    hipLaunchKernelGGL(k_enc_count, dim3(pgrid), dim3(256), 0, s, rep, flag, n_pre, ulen);
    HIPCHK(c, hipGetLastError());
    if (exclusive_scan<uint32_t>(s, ulen, n_pre, id_off, n_pre + 1) != 0) return fail(c, YABPE_E_HIP, "scan of the id counts failed");
    unsigned long long n_ids = 0;
    HIPCHK(c, hipMemcpyAsync(&n_ids, id_off + n_pre, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->enc_sums, wsums, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    TRY(dmalloc(c, &c->enc_ids, n_ids));
    if (words) { // every document's first pre-token first: the emit pass numbers the pre-tokens from it
        uint32_t *doc_pre = nullptr;
        HIPCHK(c, S.get(&doc_pre, (uint64_t)n_docs + 1));
        hipLaunchKernelGGL(k_enc_docs, dim3((n_docs + 1 + 255) / 256), dim3(256), 0, s, d_docs, n_docs, n, off, n_pre, id_off, doc_ids, doc_pre);
        if (n_pre >= ENC_WORD_SPECIAL) { // (only then can a document hold 2^31 pieces: the index would reach the flag bit)
            std::vector<uint32_t> h_pre((size_t)n_docs + 1);
            HIPCHK(c, hipMemcpyAsync(h_pre.data(), doc_pre, h_pre.size() * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            for (uint32_t d = 0; d < n_docs; ++d)
                if (h_pre[d + 1] - h_pre[d] >= ENC_WORD_SPECIAL) {
                    yabpe_encode_free(c);
                    return fail(c, YABPE_E_CAPACITY, "document %u has %u pieces: at most 2^31 - 1", d, h_pre[d + 1] - h_pre[d]);
                }
        }
        TRY(dmalloc(c, &c->enc_words, n_ids));
        hipLaunchKernelGGL(k_enc_emit_words, dim3(pgrid), dim3(256), 0, s, rep, uoff, uids, id_off, off, n_pre, doc_pre, n_docs, sflag, c->enc_ids,
                           c->enc_words);
    } else {
        hipLaunchKernelGGL(k_enc_emit, dim3(pgrid), dim3(256), 0, s, rep, uoff, uids, id_off, n_pre, c->enc_ids);
    }
    if (spans) {
        TRY(dmalloc(c, &c->enc_spans, 2 * n_ids));
        if (chars) { // the lead-byte prefix of the text, one entry per granule
            hipLaunchKernelGGL(k_enc_lead_count, dim3((uint32_t)((n_gran * 4 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, d_text, n, lead_cnt);
            HIPCHK(c, hipGetLastError());
            if (exclusive_scan<uint8_t>(s, lead_cnt, n_gran, lead_table, n_gran + 1) != 0) return fail(c, YABPE_E_HIP, "scan of the lead-byte counts failed");
            hipLaunchKernelGGL(k_enc_emit_spans<true>, dim3(pgrid), dim3(256), 0, s, rep, uoff, upos, id_off, off, n_pre, d_docs, n_docs, d_text, n,
                               lead_table, (ulonglong2 *)c->enc_spans);
        } else {
            hipLaunchKernelGGL(k_enc_emit_spans<false>, dim3(pgrid), dim3(256), 0, s, rep, uoff, upos, id_off, off, n_pre, d_docs, n_docs, d_text, n,
                               lead_table, (ulonglong2 *)c->enc_spans);
        }
    }
    if (!words) hipLaunchKernelGGL(k_enc_docs, dim3((n_docs + 1 + 255) / 256), dim3(256), 0, s, d_docs, n_docs, n, off, n_pre, id_off, doc_ids, (uint32_t *)nullptr);
    (void)hipEventRecord(c->enc_ev[7], s);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(s);
    float ms[6] = {0, 0, 0, 0, 0, 0};
    if (le == hipSuccess && se == hipSuccess) {
        (void)hipEventElapsedTime(&ms[0], c->enc_ev[0], c->enc_ev[1]);
        (void)hipEventElapsedTime(&ms[1], c->enc_ev[1], c->enc_ev[2]);
        (void)hipEventElapsedTime(&ms[2], c->enc_ev[2], c->enc_ev[3]);
        (void)hipEventElapsedTime(&ms[3], c->enc_ev[4], c->enc_ev[5]);
        (void)hipEventElapsedTime(&ms[4], c->enc_ev[6], c->enc_ev[7]);
        (void)hipEventElapsedTime(&ms[5], c->enc_ev[0], c->enc_ev[7]);
    }
    if (le != hipSuccess || se != hipSuccess) return fail(c, YABPE_E_HIP, "encoder kernels failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    auto &st = c->enc_stats;
    st.n_pretokens = n_pre;
    st.n_unique = nu;
    st.n_ids = n_ids;
    st.split_ms = ms[0];
    st.pretok_ms = ms[1];
    st.pool_ms = ms[2];
    st.words_ms = ms[3];
    st.emit_ms = ms[4];
    st.total_ms = ms[5];
    {   // counts for the statistics: long unique words and the specials taken (small host reads)
        std::vector<uint32_t> h_llen(nu);
        if (nu) HIPCHK(c, hipMemcpy(h_llen.data(), llen, nu * 4, hipMemcpyDeviceToHost));
        for (uint32_t x : h_llen) st.n_unique_long += x ? 1 : 0;
        st.n_specials = c->enc_sums[3];
    }
    c->enc_done = true;
    *out_dev_ids = c->enc_ids;
    *out_dev_doc_off = (uint64_t *)c->enc_doc;
    if (spans) *out_dev_spans = (uint64_t *)c->enc_spans;
    if (words) *out_dev_words = c->enc_words;
    *out_n_ids = n_ids;
    return YABPE_OK;
}

int yabpe_encode(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint32_t **out_dev_ids,
                 uint64_t **out_dev_doc_off, uint64_t *out_n_ids, int64_t *out_bad_pos) {
    if (!c || !out_dev_ids || !out_dev_doc_off || !out_n_ids || !out_bad_pos) return YABPE_E_INVALID;
    return encode_run(c, text, n_bytes, doc_off, n_docs, 0, out_dev_ids, out_dev_doc_off, nullptr, nullptr, out_n_ids, out_bad_pos);
}

int yabpe_encode_spans(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint32_t flags,
                       uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint64_t **out_dev_spans, uint64_t *out_n_ids, int64_t *out_bad_pos) {
    if (!c || !out_dev_ids || !out_dev_doc_off || !out_dev_spans || !out_n_ids || !out_bad_pos) return YABPE_E_INVALID;
    return encode_run(c, text, n_bytes, doc_off, n_docs, flags, out_dev_ids, out_dev_doc_off, out_dev_spans, nullptr, out_n_ids, out_bad_pos);
}

int yabpe_encode_words(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint32_t **out_dev_ids,
                       uint64_t **out_dev_doc_off, uint32_t **out_dev_words, uint64_t *out_n_ids, int64_t *out_bad_pos) {
    if (!c || !out_dev_ids || !out_dev_doc_off || !out_dev_words || !out_n_ids || !out_bad_pos) return YABPE_E_INVALID;
    return encode_run(c, text, n_bytes, doc_off, n_docs, 0, out_dev_ids, out_dev_doc_off, nullptr, out_dev_words, out_n_ids, out_bad_pos);
}

// BBPETokenizer.encode_dropout on the device (yabpe_dropout_kernels.h): the shared front, then per occurrence -- nothing is
// pooled.  The merge runs twice (count, scan, emit in place): no staging of 4 bytes per text byte.
int yabpe_encode_dropout(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, uint64_t threshold,
                         uint64_t seed, uint32_t **out_dev_ids, uint64_t **out_dev_doc_off, uint64_t *out_n_ids, int64_t *out_bad_pos) {
    if (!c || !out_dev_ids || !out_dev_doc_off || !out_n_ids || !out_bad_pos) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_ids = nullptr; *out_dev_doc_off = nullptr; *out_n_ids = 0; *out_bad_pos = -1;
    if (threshold > ENC_DROP_ALL) return fail(c, YABPE_E_INVALID, "threshold %llu: at most 2^32 (p = 1)", (unsigned long long)threshold);
    if (!c->have_enc_model) return fail(c, YABPE_E_INVALID, "no model: call yabpe_encode_set_model first");
    uint32_t G_checked = 0;
    TRY(digit_group_opt(c, &G_checked)); // (also when there is no text to split)
    uint32_t pattern_checked = 0;
    TRY(split_pattern_opt(c, G_checked, &pattern_checked));
    if (n_bytes && !text) return fail(c, YABPE_E_INVALID, "text is NULL");
    TRY(check_starts(c, doc_off, n_docs, n_bytes, "text"));
    yabpe_encode_free(c);
    c->enc_done = false;  // (the checksum fold is the pooled encoder's: none here)
    c->enc_stats = yabpe_encode_stats_t{};
    c->enc_stats.n_bytes = n_bytes;
    c->enc_stats.n_docs = n_docs;
    TRY(class_table(c));
    for (auto &e : c->enc_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    const unsigned long long n = n_bytes;
    Scratch S(c->device, c->rank);
    const uint8_t *d_text = nullptr;
    TRY(to_device(c, S, text, n, 1, &d_text));
    unsigned long long *d_docs = nullptr;
    HIPCHK(c, S.get(&d_docs, n_docs));
    HIPCHK(c, hipMemcpy(d_docs, doc_off, (size_t)n_docs * 8, hipMemcpyHostToDevice));
    TRY(dmalloc(c, &c->enc_doc, (uint64_t)n_docs + 1));
    unsigned long long *doc_ids = (unsigned long long *)c->enc_doc;
    if (n == 0) { // every document is empty
        HIPCHK(c, hipMemsetAsync(doc_ids, 0, ((size_t)n_docs + 1) * 8, s));
        TRY(dmalloc(c, &c->enc_ids, 1));
        HIPCHK(c, hipStreamSynchronize(s));
        *out_dev_ids = c->enc_ids;
        *out_dev_doc_off = (uint64_t *)c->enc_doc;
        return YABPE_OK;
    }
    EncFront F;
    TRY(encode_front(c, S, d_text, n, d_docs, n_docs, out_bad_pos, &F));
    S.release(F.meta);  // (dead from here on: the peak is the front's)
    S.release(F.flags);
    unsigned long long *const off = F.off;
    const unsigned long long n_pre = F.n_pre;
    const EncTable tab{c->enc_keys, c->enc_vals, c->enc_mask};
    const uint32_t pgrid = (uint32_t)((n_pre + 255) / 256);
    // ---- long words: their list, the walk's scratch, the walk (once: its tokens stay in the scratch for the emit)
    const unsigned long long lcap = n / (ENC_SHORT + 1) + 1;
    uint32_t *cnt = nullptr, *llist = nullptr;
    unsigned long long *id_off = nullptr, *lbase = nullptr, *ctr = nullptr;
    HIPCHK(c, S.get(&cnt, n_pre));
    HIPCHK(c, S.get(&id_off, n_pre + 1));
    HIPCHK(c, S.get(&llist, lcap));
    HIPCHK(c, S.get(&lbase, lcap));
    HIPCHK(c, S.get(&ctr, 3));  // long words, their bytes; specials met
    HIPCHK(c, hipMemsetAsync(ctr, 0, 24, s));
    hipLaunchKernelGGL(k_drop_long_list, dim3(pgrid), dim3(256), 0, s, off, n_pre, F.sflag, lcap, llist, lbase, ctr);
    HIPCHK(c, hipGetLastError());
    unsigned long long h_ctr[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h_ctr, ctr, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long n_long = std::min(h_ctr[0], lcap), lbytes = h_ctr[1];
    uint32_t *ltok = nullptr, *lnxt = nullptr, *lprv = nullptr;
    unsigned long long *lheap = nullptr;
    HIPCHK(c, S.get(&ltok, lbytes));
    HIPCHK(c, S.get(&lnxt, lbytes));
    HIPCHK(c, S.get(&lprv, lbytes));
    HIPCHK(c, S.get(&lheap, 3 * lbytes));
    HIPCHK(c, hipEventRecord(c->enc_ev[4], s));  // (the words phase: the long walks and the count pass)
    const uint32_t lgrid = (uint32_t)((n_long + 63) / 64);
    if (n_long) {
        const DropLongParams LP{d_text, off, d_docs, n_docs, llist, lbase, n_long, tab, seed, threshold, cnt, ltok, lnxt, lprv, lheap};
        hipLaunchKernelGGL(k_drop_long, dim3(lgrid), dim3(64), 0, s, LP);
    }
    DropParams W{d_text, off, n_pre, d_docs, n_docs, optv(c, "dropout_pack", 1) ? DROP_PACK : 0u, F.sflag, tab, c->enc_out_id, c->enc_sp_id,
                 c->enc_sp_has, seed, threshold, cnt, nullptr, nullptr, ctr + 2};
    const uint32_t wg = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>((n_pre + 64ull * WPB - 1) / (64ull * WPB), (unsigned long long)c->n_cu * 8));
    hipLaunchKernelGGL(k_drop_words<false>, dim3(wg), dim3(BLOCK), 0, s, W);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->enc_ev[5], s));
    // ---- emission: id offsets, the merges again with the ids written in place, the per-document offsets
    HIPCHK(c, hipEventRecord(c->enc_ev[6], s));
    if (exclusive_scan<uint32_t>(s, cnt, n_pre, id_off, n_pre + 1) != 0) return fail(c, YABPE_E_HIP, "scan of the id counts failed");
    unsigned long long n_ids = 0;
    HIPCHK(c, hipMemcpyAsync(&n_ids, id_off + n_pre, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&h_ctr[2], ctr + 2, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    TRY(dmalloc(c, &c->enc_ids, n_ids));
    W.id_off = id_off;
    W.ids = c->enc_ids;
    hipLaunchKernelGGL(k_drop_words<true>, dim3(wg), dim3(BLOCK), 0, s, W);
    if (n_long) hipLaunchKernelGGL(k_drop_long_emit, dim3(lgrid), dim3(64), 0, s, llist, lbase, n_long, ltok, id_off, c->enc_out_id, c->enc_ids);
    hipLaunchKernelGGL(k_enc_docs, dim3((n_docs + 1 + 255) / 256), dim3(256), 0, s, d_docs, n_docs, n, off, n_pre, id_off, doc_ids, (uint32_t *)nullptr);
    (void)hipEventRecord(c->enc_ev[7], s);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(s);
    if (le != hipSuccess || se != hipSuccess) return fail(c, YABPE_E_HIP, "encoder kernels failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    float ms[5] = {0, 0, 0, 0, 0};
    (void)hipEventElapsedTime(&ms[0], c->enc_ev[0], c->enc_ev[1]);
    (void)hipEventElapsedTime(&ms[1], c->enc_ev[1], c->enc_ev[2]);
    (void)hipEventElapsedTime(&ms[2], c->enc_ev[4], c->enc_ev[5]);
    (void)hipEventElapsedTime(&ms[3], c->enc_ev[6], c->enc_ev[7]);
    (void)hipEventElapsedTime(&ms[4], c->enc_ev[0], c->enc_ev[7]);
    auto &st = c->enc_stats;  // (n_unique and pool_ms stay 0: nothing is pooled; n_unique_long counts occurrences here)
    st.n_pretokens = n_pre;
    st.n_unique_long = n_long;
    st.n_specials = h_ctr[2];
    st.n_ids = n_ids;
    st.split_ms = ms[0];
    st.pretok_ms = ms[1];
    st.words_ms = ms[2];
    st.emit_ms = ms[3];
    st.total_ms = ms[4];
    *out_dev_ids = c->enc_ids;
    *out_dev_doc_off = (uint64_t *)c->enc_doc;
    *out_n_ids = n_ids;
    return YABPE_OK;
}

int yabpe_encode_stats(yabpe_ctx *c, yabpe_encode_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->enc_stats;
    return YABPE_OK;
}

int yabpe_encode_checksum(yabpe_ctx *c, uint64_t *out_sum, uint64_t *out_words, uint64_t *out_tokens) {
    if (!c) return YABPE_E_INVALID;
    if (!c->enc_done) return fail(c, YABPE_E_INVALID, "no encode has completed on this context");
    if (out_sum) *out_sum = c->enc_sums[0];
    if (out_words) *out_words = c->enc_sums[1];
    if (out_tokens) *out_tokens = c->enc_sums[2];
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- decoder
int yabpe_decode_set_model(yabpe_ctx *c, const uint8_t *vocab_bytes, const uint64_t *vocab_off, const uint32_t *vocab_ids, uint32_t n_vocab) {
    if (!c) return YABPE_E_INVALID;
    if (n_vocab && (!vocab_bytes || !vocab_off || !vocab_ids)) return fail(c, YABPE_E_INVALID, "vocab arrays are NULL");
    HIPCHK(c, hipSetDevice(c->device));
    DecTableHost t;
    const int r = dec_build_table(vocab_off, vocab_ids, n_vocab, &t);
    if (r == -1) return fail(c, YABPE_E_CAPACITY, "a token id is above %u: the decode table holds ids below 2^24", DEC_MAX_ID);
    if (r != 0) return fail(c, YABPE_E_CAPACITY, "the vocab holds %llu bytes: the decode table addresses fewer than 2^32 - 1",
                            (unsigned long long)vocab_off[n_vocab]);
    c->have_dec_model = false;
    dfree(c->dec_ent); dfree(c->dec_pool);
    c->dec_ent = nullptr; c->dec_pool = nullptr;
    const uint64_t pool_bytes = n_vocab ? vocab_off[n_vocab] : 0;
    c->dec_n = (uint32_t)(t.ent.size() / 2);
    TRY(dmalloc(c, &c->dec_ent, c->dec_n));
    TRY(dmalloc(c, &c->dec_pool, pool_bytes));
    if (c->dec_n) HIPCHK(c, hipMemcpy(c->dec_ent, t.ent.data(), t.ent.size() * 4, hipMemcpyHostToDevice));
    if (pool_bytes) HIPCHK(c, hipMemcpy(c->dec_pool, vocab_bytes, pool_bytes, hipMemcpyHostToDevice));
    c->have_dec_model = true;
    return YABPE_OK;
}

int yabpe_decode_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    dfree(c->dec_text);
    dfree(c->dec_doc);
    c->dec_text = nullptr;
    c->dec_doc = nullptr;
    return YABPE_OK;
}

int yabpe_decode(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, uint8_t **out_dev_text,
                 uint64_t **out_dev_text_off, uint64_t *out_n_bytes) {
    if (!c || !out_dev_text || !out_dev_text_off || !out_n_bytes) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_text = nullptr; *out_dev_text_off = nullptr; *out_n_bytes = 0;
    if (!c->have_dec_model) return fail(c, YABPE_E_INVALID, "no model: call yabpe_decode_set_model first");
    if (n_ids && !ids) return fail(c, YABPE_E_INVALID, "ids is NULL");
    if (!doc_off && n_docs > 1) return fail(c, YABPE_E_INVALID, "doc_off is NULL with %u documents", n_docs);
    const unsigned long long nb = (n_ids + DEC_IPB - 1) / DEC_IPB;
    if (nb > (1ull << 23)) return fail(c, YABPE_E_CAPACITY, "%llu ids in one call: at most 2^34", (unsigned long long)n_ids);
    // the document starts on the host (validated: the kernels index the ids with them) and on the device
    const bool docs_dev = doc_off && is_device_ptr(doc_off);
    if (!doc_off) n_docs = 1;
    std::vector<uint64_t> h_docs(n_docs, 0);
    if (doc_off && n_docs) {
        if (docs_dev) HIPCHK(c, hipMemcpy(h_docs.data(), doc_off, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        else memcpy(h_docs.data(), doc_off, (size_t)n_docs * 8);
    }
    TRY(check_starts(c, h_docs.data(), n_docs, n_ids, "ids"));
    yabpe_decode_free(c);
    c->dec_stats = yabpe_decode_stats_t{};
    c->dec_stats.n_ids = n_ids;
    c->dec_stats.n_docs = n_docs;
    for (auto &e : c->dec_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    Scratch S(c->device, c->rank);
    // inputs on the device (16-B aligned ids: the kernels load them 4 at a time)
    const uint32_t *d_ids = nullptr;
    TRY(to_device(c, S, ids, n_ids * 4, 16, &d_ids));
    const unsigned long long *d_docs = nullptr;
    TRY(to_device(c, S, docs_dev ? (const unsigned long long *)doc_off : (const unsigned long long *)h_docs.data(), (uint64_t)n_docs * 8, 1, &d_docs));
    TRY(dmalloc(c, &c->dec_doc, (uint64_t)n_docs + 1));
    if (n_ids == 0) { // every document is empty
        HIPCHK(c, hipMemsetAsync(c->dec_doc, 0, ((size_t)n_docs + 1) * 8, s));
        TRY(dmalloc(c, &c->dec_text, 1));
        HIPCHK(c, hipStreamSynchronize(s));
        *out_dev_text = c->dec_text;
        *out_dev_text_off = (uint64_t *)c->dec_doc;
        return YABPE_OK;
    }
    const DecTable tab{c->dec_ent, c->dec_n, c->dec_pool};
    // ---- lengths: per-block byte counts -> block output bases
    unsigned long long *bsum = nullptr, *bbase = nullptr, *counters = nullptr;
    HIPCHK(c, S.get(&bsum, nb));
    HIPCHK(c, S.get(&bbase, nb + 1));
    HIPCHK(c, S.get(&counters, 2));
    HIPCHK(c, hipEventRecord(c->dec_ev[0], s));
    HIPCHK(c, hipMemsetAsync(counters, 0, 16, s));
    hipLaunchKernelGGL(k_dec_lengths, dim3((uint32_t)nb), dim3(BLOCK), 0, s, d_ids, (unsigned long long)n_ids, tab, bsum, counters);
    HIPCHK(c, hipGetLastError());
    if (exclusive_scan<unsigned long long>(s, bsum, nb, bbase, nb + 1) != 0) return fail(c, YABPE_E_HIP, "scan of the block lengths failed");
    HIPCHK(c, hipEventRecord(c->dec_ev[1], s));
    unsigned long long G = 0;
    HIPCHK(c, hipMemcpyAsync(&G, bbase + nb, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long nt = (G + DEC_TILE - 1) / DEC_TILE;
    if (nt > (1ull << 24)) return fail(c, YABPE_E_CAPACITY, "%llu bytes of text in one call: at most 2^36", G);
    // ---- gather: token bytes -> text, document offsets
    uint8_t *gtext = nullptr;  // (scratch until it turns out to be the result)
    HIPCHK(c, S.get(&gtext, G));
    HIPCHK(c, hipEventRecord(c->dec_ev[2], s)); // (the allocation above is host work)
    hipLaunchKernelGGL(k_dec_gather, dim3((uint32_t)nb), dim3(BLOCK), 0, s,
                       DecGatherParams{d_ids, n_ids, tab, bbase, d_docs, n_docs, gtext, c->dec_doc});
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->dec_ev[3], s));
    // ---- check: output bytes per tile, U+FFFD count
    uint32_t *osum = nullptr;
    HIPCHK(c, S.get(&osum, nt));
    if (nt) hipLaunchKernelGGL(k_dec_check, dim3((uint32_t)nt), dim3(BLOCK), 0, s, DecCheckParams{gtext, G, c->dec_doc, n_docs, osum, counters});
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->dec_ev[4], s));
    unsigned long long h_cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h_cnt, counters, 16, hipMemcpyDeviceToHost, s));
    const hipError_t ce = hipStreamSynchronize(s);
    if (ce != hipSuccess) return fail(c, YABPE_E_HIP, "decoder kernels failed: %s", hipGetErrorString(ce));
    auto &st = c->dec_stats;
    st.n_unknown = h_cnt[0];
    st.n_gathered = G;
    st.n_replacements = h_cnt[1];
    float ms[5] = {0, 0, 0, 0, 0};
    (void)hipEventElapsedTime(&ms[0], c->dec_ev[0], c->dec_ev[1]);
    (void)hipEventElapsedTime(&ms[1], c->dec_ev[2], c->dec_ev[3]);
    (void)hipEventElapsedTime(&ms[2], c->dec_ev[3], c->dec_ev[4]);
    hipEvent_t last = c->dec_ev[4];
    unsigned long long n_out = G;
    if (h_cnt[1] == 0) { // valid UTF-8: the gathered text is the result
        c->dec_text = S.take(gtext);
    } else {
        // ---- repair: tile output bases, the rewrite with U+FFFD, the repaired documents
        S.adopt(c->dec_doc); // (the gathered text and its offsets are scratch from here on)
        const unsigned long long *gdoc = c->dec_doc;
        c->dec_doc = nullptr;
        unsigned long long *rbase = nullptr, *nbad = nullptr;
        uint32_t *docbad = nullptr;
        HIPCHK(c, S.get(&rbase, nt + 1));
        HIPCHK(c, S.get(&docbad, n_docs));
        HIPCHK(c, S.get(&nbad, (uint64_t)n_docs + 1));
        TRY(dmalloc(c, &c->dec_doc, (uint64_t)n_docs + 1));
        HIPCHK(c, hipEventRecord(c->dec_ev[5], s));
        HIPCHK(c, hipMemsetAsync(docbad, 0, (size_t)n_docs * 4, s));
        int r = exclusive_scan<uint32_t>(s, osum, nt, rbase, nt + 1);
        if (r == 0) r = hipMemcpyAsync(&n_out, rbase + nt, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess ? 0 : -1;
        if (r == 0) r = dmalloc(c, &c->dec_text, n_out);
        if (r == 0) {
            hipLaunchKernelGGL(k_dec_repair, dim3((uint32_t)nt), dim3(BLOCK), 0, s,
                               DecRepairParams{gtext, G, gdoc, n_docs, rbase, c->dec_text, c->dec_doc, docbad});
            r = hipGetLastError() == hipSuccess ? 0 : -1;
        }
        if (r == 0) r = exclusive_scan<uint32_t>(s, docbad, n_docs, nbad, (uint64_t)n_docs + 1);
        HIPCHK(c, hipEventRecord(c->dec_ev[6], s));
        unsigned long long h_bad = 0;
        if (r == 0) r = hipMemcpyAsync(&h_bad, nbad + n_docs, 8, hipMemcpyDeviceToHost, s) == hipSuccess ? 0 : -1;
        const hipError_t se = hipStreamSynchronize(s);
        if (r != 0 || se != hipSuccess) {
            yabpe_decode_free(c);
            return fail(c, YABPE_E_HIP, "decoder repair failed%s%s", se != hipSuccess ? ": " : "", se != hipSuccess ? hipGetErrorString(se) : "");
        }
        st.n_docs_repaired = h_bad;
        (void)hipEventElapsedTime(&ms[3], c->dec_ev[5], c->dec_ev[6]);
        last = c->dec_ev[6];
    }
    (void)hipEventElapsedTime(&ms[4], c->dec_ev[0], last);
    st.n_bytes = n_out;
    st.lengths_ms = ms[0];
    st.gather_ms = ms[1];
    st.check_ms = ms[2];
    st.repair_ms = ms[3];
    st.total_ms = ms[4];
    *out_dev_text = c->dec_text;
    *out_dev_text_off = (uint64_t *)c->dec_doc;
    *out_n_bytes = n_out;
    return YABPE_OK;
}

int yabpe_decode_stats(yabpe_ctx *c, yabpe_decode_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->dec_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- fixed-shape batches
int yabpe_layout_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    for (auto &p : c->lay_buf) {
        dfree(p);
        p = nullptr;
    }
    return YABPE_OK;
}

int yabpe_layout_pad(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const yabpe_layout_t *lay,
                     uint32_t **out_dev_rows, uint32_t **out_dev_len, uint32_t *out_row_len) {
    if (!c || !out_dev_rows || !out_dev_len || !out_row_len) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_rows = nullptr; *out_dev_len = nullptr; *out_row_len = 0;
    if (lay && lay->row_len && lay->row_len < lay_n_added(lay->flags & LAY_PAD_FLAGS))
        return fail(c, YABPE_E_INVALID, "row_len %u cannot hold BOS and EOS", lay->row_len);
    if (lay && (unsigned long long)lay->row_len * n_docs > LAY_MAX_SLOTS)
        return fail(c, YABPE_E_CAPACITY, "%u rows of %u slots: at most 2^36 slots in one call", n_docs, lay->row_len);
    LayoutCall Q(c);
    TRY(Q.begin(ids, n_ids, doc_off, &n_docs, nullptr, lay, LAY_PAD_FLAGS));
    // ---- lengths: kept length per document, the longest sequence, what the cut drops
    TRY(dmalloc(c, &c->lay_buf[LB_ROW_DOC], n_docs));
    TRY(Q.count_begin());
    hipLaunchKernelGGL(k_lay_lengths<false>, dim3(cdiv64(n_docs, BLOCK)), dim3(BLOCK), 0, Q.s,
                       LayLenParams{Q.d_docs, n_docs, n_ids, lay->row_len, lay->flags, c->lay_buf[LB_ROW_DOC], nullptr, Q.counters});
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->lay_ev[1], Q.s));
    TRY(Q.row_offsets(nullptr, 0, nullptr, nullptr));
    const unsigned long long L = lay->row_len ? lay->row_len : Q.h_cnt[0];
    const unsigned long long n_slots = L * n_docs;
    if (L > 0xFFFFFFFFull || n_slots > LAY_MAX_SLOTS) {
        yabpe_layout_free(c);
        return fail(c, YABPE_E_CAPACITY, "%u rows of %llu slots (the longest sequence): at most 2^36 slots of at most 2^32 - 1 a row", n_docs, L);
    }
    // ---- write
    TRY(dmalloc(c, &c->lay_buf[LB_ROWS], n_slots));
    HIPCHK(c, hipEventRecord(c->lay_ev[2], Q.s));
    if (n_slots)
        hipLaunchKernelGGL(k_lay_pad_write, dim3(cdiv64(n_slots, LAY_PIECE)), dim3(BLOCK), 0, Q.s,
                           LayPadParams{Q.d_ids, Q.d_docs, n_docs, n_ids, (uint32_t)L, lay->flags, Q.K(), c->lay_buf[LB_ROWS], n_slots});
    TRY(Q.end(n_docs, L, n_slots));
    *out_dev_rows = c->lay_buf[LB_ROWS];
    *out_dev_len = c->lay_buf[LB_ROW_DOC];
    *out_row_len = (uint32_t)L;
    return YABPE_OK;
}

int yabpe_layout_pack(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const yabpe_layout_t *lay,
                      uint32_t **out_dev_ids, uint32_t **out_dev_doc, uint32_t **out_dev_pos, uint64_t *out_n_rows) {
    if (!c || !out_dev_ids || !out_dev_doc || !out_dev_pos || !out_n_rows) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_ids = nullptr; *out_dev_doc = nullptr; *out_dev_pos = nullptr; *out_n_rows = 0;
    if (lay && lay->row_len == 0) return fail(c, YABPE_E_INVALID, "row_len is 0: a packed row holds at least one slot");
    LayoutCall Q(c);
    TRY(Q.begin(ids, n_ids, doc_off, &n_docs, nullptr, lay, LAY_PACK_FLAGS));
    const unsigned long long total = n_ids + (unsigned long long)lay_n_added(lay->flags) * n_docs;
    if (total > LAY_MAX_SLOTS) return fail(c, YABPE_E_CAPACITY, "a stream of %llu entries: at most 2^36 slots in one call", total);
    const unsigned long long n_rows = lay_pack_rows(total, lay->row_len, lay->flags), n_slots = n_rows * lay->row_len;
    // ---- lengths: the stream offsets (closed form) and the longest sequence
    unsigned long long *soff = nullptr;
    HIPCHK(c, Q.S.get(&soff, (uint64_t)n_docs + 1));
    TRY(Q.count_begin());
    hipLaunchKernelGGL(k_lay_lengths<true>, dim3(cdiv64(n_docs, BLOCK)), dim3(BLOCK), 0, Q.s,
                       LayLenParams{Q.d_docs, n_docs, n_ids, lay->row_len, lay->flags, nullptr, soff, Q.counters});
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->lay_ev[1], Q.s));
    TRY(Q.row_offsets(nullptr, 0, nullptr, nullptr));
    if (Q.h_cnt[0] > 0xFFFFFFFFull) return fail(c, YABPE_E_CAPACITY, "a document of %llu stream entries: positions are u32", Q.h_cnt[0]);
    // ---- write
    for (int k : {LB_ROWS, LB_ROW_DOC, LB_ROW_START}) TRY(dmalloc(c, &c->lay_buf[k], n_slots));
    HIPCHK(c, hipEventRecord(c->lay_ev[2], Q.s));
    if (n_slots)
        hipLaunchKernelGGL(k_lay_pack_write, dim3(cdiv64(n_slots, LAY_PIECE)), dim3(BLOCK), 0, Q.s,
                           LayPackParams{Q.d_ids, soff, n_docs, total, n_slots, lay->flags, Q.K(), c->lay_buf[LB_ROWS], c->lay_buf[LB_ROW_DOC],
                                         c->lay_buf[LB_ROW_START]});
    TRY(Q.end());
    auto &st = c->lay_stats;
    st.n_rows = n_rows;
    st.row_len = lay->row_len;
    st.n_ids_dropped = total > n_slots ? total - n_slots : 0;
    st.n_pad_slots = n_slots > total ? n_slots - total : 0;
    *out_dev_ids = c->lay_buf[LB_ROWS];
    *out_dev_doc = c->lay_buf[LB_ROW_DOC];
    *out_dev_pos = c->lay_buf[LB_ROW_START];
    *out_n_rows = n_rows;
    return YABPE_OK;
}

int yabpe_layout_windows(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *spans,
                         const yabpe_layout_t *lay, uint32_t stride, yabpe_windows_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out = yabpe_windows_t{};
    const uint32_t added = lay ? lay_n_added(lay->flags & LAY_WIN_FLAGS) : 0u;
    if (lay && lay->row_len <= added) return fail(c, YABPE_E_INVALID, "row_len %u leaves no slot for content beside BOS and EOS", lay->row_len);
    if (lay && stride >= lay->row_len - added)
        return fail(c, YABPE_E_INVALID, "stride %u: consecutive rows of %u content slots must advance by at least one", stride, lay->row_len - added);
    LayoutCall Q(c);
    TRY(Q.begin(ids, n_ids, doc_off, &n_docs, spans, lay, LAY_WIN_FLAGS));
    const uint32_t L = lay->row_len, C = L - added, step = C - stride;
    // ---- count + scan: the rows of every document, their exclusive scan, the call's counters
    unsigned long long *cnt = nullptr, *row_off = nullptr, n_rows = 0, n_slots = 0;
    HIPCHK(c, Q.S.get(&cnt, n_docs));
    HIPCHK(c, Q.S.get(&row_off, (uint64_t)n_docs + 1));
    TRY(Q.count_begin());
    hipLaunchKernelGGL(k_lay_win_count, dim3(cdiv64(n_docs, BLOCK)), dim3(BLOCK), 0, Q.s,
                       LayWinCountParams{Q.d_docs, n_docs, n_ids, C, step, added, cnt, Q.counters});
    HIPCHK(c, hipGetLastError());
    TRY(Q.row_offsets(cnt, n_docs, row_off, &n_rows));
    TRY(Q.row_budget("row_start is", n_rows, &n_slots));
    // ---- rows: the record of every output row
    ulonglong2 *rec = nullptr;
    HIPCHK(c, Q.S.get(&rec, n_rows));
    TRY(dmalloc(c, &c->lay_buf[LB_ROWS], n_slots));
    for (int k : {LB_ROW_DOC, LB_ROW_START, LB_ROW_LEN}) TRY(dmalloc(c, &c->lay_buf[k], n_rows));
    if (spans) TRY(dmalloc(c, &c->lay_buf[LB_SPANS], 4 * n_slots));  // (16 B a slot)
    hipLaunchKernelGGL(k_lay_win_rows, dim3(cdiv64(n_rows, BLOCK)), dim3(BLOCK), 0, Q.s,
                       LayWinRowsParams{Q.d_docs, n_docs, n_ids, row_off, n_rows, C, step, added, c->lay_buf[LB_ROW_DOC], c->lay_buf[LB_ROW_START],
                                        c->lay_buf[LB_ROW_LEN], rec});
    // ---- write
    TRY(Q.write(LayWinRow{}, rec, n_rows, n_slots));
    TRY(Q.end(n_rows, L, n_slots));  // (windows drop no ids: that counter stays 0)
    out->rows = c->lay_buf[LB_ROWS];
    out->row_doc = c->lay_buf[LB_ROW_DOC];
    out->row_start = c->lay_buf[LB_ROW_START];
    out->row_len = c->lay_buf[LB_ROW_LEN];
    out->spans = (uint64_t *)c->lay_buf[LB_SPANS];
    out->n_rows = n_rows;
    return YABPE_OK;
}

int yabpe_layout_pairs(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *spans,
                       const yabpe_layout_t *lay, const yabpe_pairs_t *pairs, yabpe_pair_rows_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out = yabpe_pair_rows_t{};
    if (!lay) return fail(c, YABPE_E_INVALID, "layout is NULL");
    if (!pairs) return fail(c, YABPE_E_INVALID, "pairs is NULL");
    TRY(layout_flags(c, lay, LAY_PAIR_FLAGS));  // (ahead of begin(): the checks below read the flags, and no pairs return before it)
    if (pairs->n_sep > LAY_PAIRS_MAX_SEP) return fail(c, YABPE_E_INVALID, "n_sep %u: at most %u separators between the two sides", pairs->n_sep, LAY_PAIRS_MAX_SEP);
    if (pairs->mode > LAY_PAIRS_WINDOWS) return fail(c, YABPE_E_INVALID, "unknown pairs mode %u", pairs->mode);
    const uint32_t added = lay_n_added(lay->flags) + pairs->n_sep;
    if (lay->row_len <= added)
        return fail(c, YABPE_E_INVALID, "row_len %u leaves no slot for content beside BOS, EOS and %u separators", lay->row_len, pairs->n_sep);
    const uint32_t L = lay->row_len, C = L - added;
    if (pairs->mode != LAY_PAIRS_WINDOWS && pairs->stride) return fail(c, YABPE_E_INVALID, "stride %u: only windows mode takes a stride", pairs->stride);
    if (pairs->stride >= C)
        return fail(c, YABPE_E_INVALID, "stride %u: a row of %u content slots must keep one more than the stride for the second side", pairs->stride, C);
    if (n_docs & 1u) return fail(c, YABPE_E_INVALID, "%u documents: documents 2p and 2p + 1 are pair p, so their number is even", n_docs);
    const uint32_t n_pairs = n_docs / 2;
    if ((unsigned long long)n_pairs * L > LAY_MAX_SLOTS) // (every pair has at least one row)
        return fail(c, YABPE_E_CAPACITY, "%u pairs in rows of %u slots: at most 2^36 slots in one call", n_pairs, L);
    if (n_docs == 0) { // no pairs: no rows
        yabpe_layout_free(c);
        c->lay_stats = yabpe_layout_stats_t{};
        c->lay_stats.row_len = L;
        return YABPE_OK;
    }
    LayoutCall Q(c);
    TRY(Q.begin(ids, n_ids, doc_off, &n_docs, spans, lay, LAY_PAIR_FLAGS));
    const LayPairShape shape{C, pairs->mode, pairs->stride, pairs->n_sep, added};
    // ---- count (+ scan in windows mode: elsewhere a pair has one row and the scan would be the identity)
    unsigned long long *cnt = nullptr, *row_off = nullptr, n_rows = n_pairs, n_slots = 0;
    if (pairs->mode == LAY_PAIRS_WINDOWS) {
        HIPCHK(c, Q.S.get(&cnt, n_pairs));
        HIPCHK(c, Q.S.get(&row_off, (uint64_t)n_pairs + 1));
    }
    TRY(Q.count_begin());
    hipLaunchKernelGGL(k_lay_pair_count, dim3(cdiv64(n_pairs, BLOCK)), dim3(BLOCK), 0, Q.s, LayPairCountParams{Q.d_docs, n_docs, n_ids, shape, cnt, Q.counters});
    HIPCHK(c, hipGetLastError());
    TRY(Q.row_offsets(cnt, n_pairs, row_off, &n_rows));
    TRY(Q.row_budget("row_start and the kept lengths are", n_rows, &n_slots));
    // ---- rows: the record of every output row
    LayPairRec *rec = nullptr;
    HIPCHK(c, Q.S.get(&rec, n_rows));
    TRY(dmalloc(c, &c->lay_buf[LB_ROWS], n_slots));
    for (int k : {LB_ROW_DOC, LB_ROW_START, LB_ROW_LEN, LB_SECOND_LEN}) TRY(dmalloc(c, &c->lay_buf[k], n_rows));
    TRY(dmalloc(c, &c->lay_buf[LB_TYPES], (n_slots + 3) / 4));       // (a byte a slot)
    if (spans) TRY(dmalloc(c, &c->lay_buf[LB_SPANS], 4 * n_slots));  // (16 B a slot)
    hipLaunchKernelGGL(k_lay_pair_rows, dim3(cdiv64(n_rows, BLOCK)), dim3(BLOCK), 0, Q.s,
                       LayPairRowsParams{Q.d_docs, n_docs, n_ids, row_off, n_rows, shape, c->lay_buf[LB_ROW_DOC], c->lay_buf[LB_ROW_START],
                                         c->lay_buf[LB_ROW_LEN], c->lay_buf[LB_SECOND_LEN], rec});
    // ---- write
    TRY(Q.write(LayPairRow{pairs->n_sep, pairs->sep_id}, rec, n_rows, n_slots));
    TRY(Q.end(n_rows, L, n_slots));
    out->rows = c->lay_buf[LB_ROWS];
    out->types = (uint8_t *)c->lay_buf[LB_TYPES];
    out->row_pair = c->lay_buf[LB_ROW_DOC];
    out->row_start = c->lay_buf[LB_ROW_START];
    out->first_len = c->lay_buf[LB_ROW_LEN];
    out->second_len = c->lay_buf[LB_SECOND_LEN];
    out->spans = (uint64_t *)c->lay_buf[LB_SPANS];
    out->n_rows = n_rows;
    return YABPE_OK;
}

int yabpe_layout_fit(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const yabpe_layout_t *lay,
                     yabpe_fit_rows_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out = yabpe_fit_rows_t{};
    if (!lay) return fail(c, YABPE_E_INVALID, "layout is NULL");
    TRY(layout_flags(c, lay, LAY_FIT_FLAGS));  // (ahead of begin(): the checks below read the flags)
    if (lay->row_len == 0) return fail(c, YABPE_E_INVALID, "row_len is 0: a row holds at least one slot");
    if (lay->row_len < lay_n_added(lay->flags)) return fail(c, YABPE_E_INVALID, "row_len %u cannot hold BOS and EOS", lay->row_len);
    if (lay->row_len > FIT_MAX_ROW) return fail(c, YABPE_E_INVALID, "row_len %u: at most 2^24 - 1 slots a row", lay->row_len);
    const uint32_t C = lay->row_len;
    if (n_docs == 0) { // no documents: no rows
        yabpe_layout_free(c);
        c->lay_stats = yabpe_layout_stats_t{};
        c->lay_stats.row_len = C;
        return YABPE_OK;
    }
    LayoutCall Q(c);
    TRY(Q.begin(ids, n_ids, doc_off, &n_docs, nullptr, lay, LAY_FIT_FLAGS));
    // ---- lengths: the key n_d of every document, their histogram, the call's counters; then the documents stably by key
    uint32_t *key = nullptr, *hist = nullptr;
    HIPCHK(c, Q.S.get(&key, n_docs));
    HIPCHK(c, Q.S.get(&hist, (uint64_t)C + 1));
    std::vector<uint32_t> h_hist((size_t)C + 1, 0);
    TRY(Q.count_begin());
    HIPCHK(c, hipMemsetAsync(hist, 0, ((size_t)C + 1) * 4, Q.s));
    const FitLenParams LP{Q.d_docs, n_docs, n_ids, C, lay->flags, key, hist, Q.counters};
    if (C < (uint32_t)FIT_HIST_LDS)
        hipLaunchKernelGGL(k_fit_lengths<true>, dim3(cdiv64(n_docs, BLOCK)), dim3(BLOCK), 0, Q.s, LP);
    else
        hipLaunchKernelGGL(k_fit_lengths<false>, dim3(cdiv64(n_docs, BLOCK)), dim3(BLOCK), 0, Q.s, LP);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_hist.data(), hist, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost, Q.s));
    TRY(Q.row_offsets(nullptr, 0, nullptr, nullptr));
    const uint32_t max_key = (uint32_t)std::min<unsigned long long>(Q.h_cnt[0], C);  // 0: every sequence is empty, no rows
    const uint32_t *sorted = nullptr;
    if (max_key) TRY(fit_sort(c, Q.S, Q.s, key, n_docs, fit_sort_passes(max_key), &sorted));
    HIPCHK(c, hipEventRecord(c->lay_ev[1], Q.s));
    // ---- plan (host, beside the sort): histogram -> shapes, rows, places
    FitPlan plan;
    if (max_key) fit_plan(h_hist.data(), C, &plan);
    const unsigned long long n_rows = plan.n_rows;
    if (n_rows > LAY_MAX_SLOTS / C) return fail(c, YABPE_E_CAPACITY, "%llu rows of %u slots: at most 2^36 slots in one call", n_rows, C);
    const unsigned long long n_slots = n_rows * C;
    unsigned long long *d_first = nullptr;
    uint32_t *d_place = nullptr;
    FitPlace *d_pl = nullptr;
    if (n_rows) {
        HIPCHK(c, Q.S.get(&d_first, plan.first.size()));
        HIPCHK(c, Q.S.get(&d_place, plan.place.size()));
        HIPCHK(c, Q.S.get(&d_pl, plan.pl.size()));
        HIPCHK(c, hipMemcpyAsync(d_first, plan.first.data(), plan.first.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, Q.s));
        HIPCHK(c, hipMemcpyAsync(d_place, plan.place.data(), plan.place.size() * sizeof(uint32_t), hipMemcpyHostToDevice, Q.s));
        HIPCHK(c, hipMemcpyAsync(d_pl, plan.pl.data(), plan.pl.size() * sizeof(FitPlace), hipMemcpyHostToDevice, Q.s));
    }
    // ---- write
    for (int k : {LB_ROWS, LB_ROW_DOC, LB_ROW_START}) TRY(dmalloc(c, &c->lay_buf[k], n_slots));
    TRY(dmalloc(c, &c->lay_buf[LB_ROW_LEN], n_rows));
    HIPCHK(c, hipEventRecord(c->lay_ev[2], Q.s));
    if (n_slots)
        hipLaunchKernelGGL(k_fit_write, dim3(cdiv64(n_slots, LAY_PIECE)), dim3(BLOCK), 0, Q.s,
                           FitWriteParams{Q.d_ids, Q.d_docs, n_docs, n_ids, sorted, d_first, d_place, d_pl, plan.n_shapes(), n_slots, C, lay->flags,
                                          Q.K(), c->lay_buf[LB_ROWS], c->lay_buf[LB_ROW_DOC], c->lay_buf[LB_ROW_START], c->lay_buf[LB_ROW_LEN]});
    TRY(Q.end(n_rows, C, n_slots));
    out->ids = c->lay_buf[LB_ROWS];
    out->doc = c->lay_buf[LB_ROW_DOC];
    out->pos = c->lay_buf[LB_ROW_START];
    out->used = c->lay_buf[LB_ROW_LEN];
    out->n_rows = n_rows;
    return YABPE_OK;
}

int yabpe_layout_stats(yabpe_ctx *c, yabpe_layout_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->lay_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- masked-language-model batches
int yabpe_mask_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    dfree(c->mask_ids);
    dfree(c->mask_labels);
    c->mask_ids = nullptr;
    c->mask_labels = nullptr;
    return YABPE_OK;
}

// BBPETokenizer.mask_tokens on the device (yabpe_mask_kernels.h; the rule: mask_logic.h).  mask_ev[0..3] bracket the call's
// device work, [1..2] the kernel.  A call that the checks refuse has freed nothing.
int yabpe_mask(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *words,
               const yabpe_mask_t *mask, uint32_t **out_dev_ids, uint32_t **out_dev_labels) {
    if (!c || !out_dev_ids || !out_dev_labels) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_ids = nullptr; *out_dev_labels = nullptr;
    if (!mask) return fail(c, YABPE_E_INVALID, "mask is NULL");
    const MaskRule R{mask->select_threshold, mask->mask_threshold, mask->random_threshold, mask->mask_id, mask->n_random};
    if (!mask_rule_valid(R))
        return fail(c, YABPE_E_INVALID, "thresholds %llu, %llu, %llu with n_random %u: each at most 2^32, mask + random at most 2^32, n_random >= 1 with random > 0",
                    (unsigned long long)R.select, (unsigned long long)R.mask, (unsigned long long)R.random, R.n_random);
    if (mask->flags & ~YABPE_MASK_WHOLE_WORD) return fail(c, YABPE_E_INVALID, "unknown mask flags 0x%x", mask->flags);
    const bool whole_word = (mask->flags & YABPE_MASK_WHOLE_WORD) != 0;
    if (whole_word && !words) return fail(c, YABPE_E_INVALID, "YABPE_MASK_WHOLE_WORD needs the words array");
    if (n_ids && !ids) return fail(c, YABPE_E_INVALID, "ids is NULL");
    if (n_ids > LAY_MAX_SLOTS) return fail(c, YABPE_E_CAPACITY, "%llu ids: at most 2^36 in one call", (unsigned long long)n_ids);
    if (!doc_off && n_docs > 1) return fail(c, YABPE_E_INVALID, "doc_off is NULL with %u documents", n_docs);
    // the document starts on the host (validated: the kernel indexes the table with what it finds in it) and on the device
    const bool docs_dev = doc_off && is_device_ptr(doc_off);
    if (!doc_off) n_docs = 1;
    std::vector<uint64_t> h_docs(n_docs, 0);
    if (doc_off && n_docs) {
        if (docs_dev) HIPCHK(c, hipMemcpy(h_docs.data(), doc_off, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        else memcpy(h_docs.data(), doc_off, (size_t)n_docs * 8);
    }
    TRY(check_starts(c, h_docs.data(), n_docs, n_ids, "ids"));
    yabpe_mask_free(c);
    c->mask_stats = yabpe_mask_stats_t{};
    c->mask_stats.n_ids = n_ids;
    c->mask_stats.n_docs = n_docs;
    for (auto &e : c->mask_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    Scratch S(c->device, c->rank);
    const uint32_t *d_ids = nullptr, *d_words = nullptr;
    const unsigned long long *d_docs = nullptr;
    unsigned long long *counters = nullptr;
    TRY(to_device(c, S, ids, n_ids * 4, 4, &d_ids));
    TRY(to_device(c, S, docs_dev ? (const unsigned long long *)doc_off : (const unsigned long long *)h_docs.data(), (uint64_t)n_docs * 8, 8, &d_docs));
    if (words) TRY(to_device(c, S, words, n_ids * 4, 4, &d_words));
    constexpr uint32_t N_COUNTERS = MASK_SHARDS * MASK_SHARD_STRIDE;  // (the kernel's copies of the counters, summed below)
    HIPCHK(c, S.get(&counters, N_COUNTERS));
    TRY(dmalloc(c, &c->mask_ids, n_ids));
    TRY(dmalloc(c, &c->mask_labels, n_ids));
    HIPCHK(c, hipEventRecord(c->mask_ev[0], s));
    HIPCHK(c, hipMemsetAsync(counters, 0, N_COUNTERS * 8, s));
    HIPCHK(c, hipEventRecord(c->mask_ev[1], s));
    if (n_ids)
        hipLaunchKernelGGL(k_mask, dim3(cdiv64(n_ids, MASK_BLOCK)), dim3(MASK_BLOCK), 0, s,
                           MaskParams{d_ids, n_ids, d_docs, n_docs, n_ids ? d_words : nullptr, mask->seed, mask->first_doc, R, mask->ignore,
                                      whole_word ? 1u : 0u, c->mask_ids, c->mask_labels, counters});
    const hipError_t le = hipGetLastError();
    (void)hipEventRecord(c->mask_ev[2], s);
    unsigned long long h_all[N_COUNTERS] = {0}, h_cnt[MASK_KINDS] = {0, 0, 0, 0};
    (void)hipMemcpyAsync(h_all, counters, N_COUNTERS * 8, hipMemcpyDeviceToHost, s);
    (void)hipEventRecord(c->mask_ev[3], s);
    const hipError_t se = hipStreamSynchronize(s);
    if (le != hipSuccess || se != hipSuccess) {
        yabpe_mask_free(c);
        return fail(c, YABPE_E_HIP, "mask kernel failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    }
    for (uint32_t b = 0; b < MASK_SHARDS; ++b)
        for (uint32_t k = 0; k < MASK_KINDS; ++k) h_cnt[k] += h_all[b * MASK_SHARD_STRIDE + k];
    float ms[3] = {0, 0, 0};
    auto &st = c->mask_stats;
    st.total_ms = pass_times(c->mask_ev, 3, ms);
    st.mask_ms = ms[1];
    st.n_protected = h_cnt[MASK_PROTECTED];
    st.n_masked = h_cnt[MASK_MASKED];
    st.n_random = h_cnt[MASK_RANDOM];
    st.n_kept = h_cnt[MASK_KEPT];
    st.n_selected = st.n_masked + st.n_random + st.n_kept;
    *out_dev_ids = c->mask_ids;
    *out_dev_labels = c->mask_labels;
    return YABPE_OK;
}

int yabpe_mask_stats(yabpe_ctx *c, yabpe_mask_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->mask_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- span-corruption batches
int yabpe_span_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    dfree(c->span_in);
    dfree(c->span_tgt);
    dfree(c->span_in_off);
    dfree(c->span_tgt_off);
    c->span_in = c->span_tgt = nullptr;
    c->span_in_off = c->span_tgt_off = nullptr;
    return YABPE_OK;
}

// BBPETokenizer.corrupt_spans on the device (yabpe_span_kernels.h; the rule: span_logic.h).  span_ev[0..5] bracket the call's
// device work: [1..2] the flags pass, [2..3] run numbers and slots, [3..4] positions and offsets, [4..5] the write.  The outputs
// are allocated after [4], once the totals of the scans are on the host, so [4..5] holds that read-back and the allocation too,
// as [2..4] hold the synchronisations of exclusive_scan.  A call that the checks refuse has freed nothing.
int yabpe_span_corrupt(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *words,
                       const yabpe_span_t *span, uint32_t **out_dev_in, uint64_t **out_dev_in_off, uint64_t *out_n_in, uint32_t **out_dev_tgt,
                       uint64_t **out_dev_tgt_off, uint64_t *out_n_tgt) {
    if (!c || !out_dev_in || !out_dev_in_off || !out_n_in || !out_dev_tgt || !out_dev_tgt_off || !out_n_tgt) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_in = *out_dev_tgt = nullptr;
    *out_dev_in_off = *out_dev_tgt_off = nullptr;
    *out_n_in = *out_n_tgt = 0;
    if (!span) return fail(c, YABPE_E_INVALID, "span is NULL");
    static_assert(YABPE_SPAN_MAX_LEN == SPAN_MAX_LEN, "the header's and the rule's largest span length");
    unsigned long long h_len[SPAN_MAX_LEN - 1] = {0};
    for (uint32_t k = 0; k + 1 < SPAN_MAX_LEN; ++k) h_len[k] = span->len_threshold[k];
    if (!span_rule_valid(span->open_threshold, h_len, span->max_len))
        return fail(c, YABPE_E_INVALID, "open_threshold %llu, max_len %u: thresholds at most 2^32, len_threshold non-increasing, max_len in 1 .. %u",
                    (unsigned long long)span->open_threshold, span->max_len, SPAN_MAX_LEN);
    if (span->flags & ~(YABPE_SPAN_WHOLE_WORD | YABPE_SPAN_FINAL_SENTINEL)) return fail(c, YABPE_E_INVALID, "unknown span flags 0x%x", span->flags);
    const bool whole_word = (span->flags & YABPE_SPAN_WHOLE_WORD) != 0, final_sentinel = (span->flags & YABPE_SPAN_FINAL_SENTINEL) != 0;
    if (span->n_sentinels < (final_sentinel ? 2u : 1u) || !span->sentinels)
        return fail(c, YABPE_E_INVALID, "%u sentinels: at least %u", span->sentinels ? span->n_sentinels : 0u, final_sentinel ? 2u : 1u);
    if (whole_word && !words) return fail(c, YABPE_E_INVALID, "YABPE_SPAN_WHOLE_WORD needs the words array");
    if (n_ids && !ids) return fail(c, YABPE_E_INVALID, "ids is NULL");
    if (n_ids > LAY_MAX_SLOTS) return fail(c, YABPE_E_CAPACITY, "%llu ids: at most 2^36 in one call", (unsigned long long)n_ids);
    if (!doc_off && n_docs > 1) return fail(c, YABPE_E_INVALID, "doc_off is NULL with %u documents", n_docs);
    // the document starts on the host (validated: the kernels index the table with what they find in it) and on the device
    const bool docs_dev = doc_off && is_device_ptr(doc_off);
    if (!doc_off) n_docs = 1;
    std::vector<uint64_t> h_docs(n_docs, 0);
    if (doc_off && n_docs) {
        if (docs_dev) HIPCHK(c, hipMemcpy(h_docs.data(), doc_off, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        else memcpy(h_docs.data(), doc_off, (size_t)n_docs * 8);
    }
    TRY(check_starts(c, h_docs.data(), n_docs, n_ids, "ids"));
    yabpe_span_free(c);
    c->span_stats = yabpe_span_stats_t{};
    c->span_stats.n_ids = n_ids;
    c->span_stats.n_docs = n_docs;
    for (auto &e : c->span_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    Scratch S(c->device, c->rank);
    constexpr uint32_t N_COUNTERS = MASK_SHARDS * MASK_SHARD_STRIDE;
    SpanParams P{};
    const unsigned long long *d_len = nullptr;
    P.n_ids = n_ids;
    P.n_docs = n_docs;
    TRY(to_device(c, S, ids, n_ids * 4, 4, &P.ids));
    TRY(to_device(c, S, docs_dev ? (const unsigned long long *)doc_off : (const unsigned long long *)h_docs.data(), (uint64_t)n_docs * 8, 8, &P.doc_off));
    if (words && n_ids) TRY(to_device(c, S, words, n_ids * 4, 4, &P.words));
    TRY(to_device(c, S, (const unsigned long long *)h_len, sizeof(h_len), 8, &d_len));
    TRY(to_device(c, S, span->sentinels, (uint64_t)span->n_sentinels * 4, 4, &P.sentinels));
    P.seed = span->seed;
    P.first_doc = span->first_doc;
    P.rule = SpanRule{span->open_threshold, d_len, span->max_len};
    P.max_doc_ids = span->max_doc_ids;
    P.K = span->n_sentinels - (final_sentinel ? 1u : 0u);
    P.whole_word = whole_word ? 1u : 0u;
    P.final_sentinel = final_sentinel ? 1u : 0u;
    HIPCHK(c, S.get(&P.flags, n_ids));
    HIPCHK(c, S.get(&P.start, n_ids));
    HIPCHK(c, S.get(&P.c_in, n_ids));
    HIPCHK(c, S.get(&P.c_tgt, n_ids));
    HIPCHK(c, S.get(&P.run, n_ids + 1));
    HIPCHK(c, S.get(&P.in_pos, n_ids + 1));
    HIPCHK(c, S.get(&P.tgt_pos, n_ids + 1));
    HIPCHK(c, S.get(&P.counters, N_COUNTERS));
    TRY(dmalloc(c, &c->span_in_off, (uint64_t)n_docs + 1));
    TRY(dmalloc(c, &c->span_tgt_off, (uint64_t)n_docs + 1));
    P.in_off = c->span_in_off;
    P.tgt_off = c->span_tgt_off;
    const dim3 grid(cdiv64(n_ids, SPAN_BLOCK)), block(SPAN_BLOCK);
    // the call fails: nothing of it is left in the context (the stream is drained first: Scratch hands its buffers back)
    auto hip_fail = [&](const char *what, hipError_t e) {
        (void)hipStreamSynchronize(s);
        yabpe_span_free(c);
        return fail(c, YABPE_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    unsigned long long h_tot[3] = {0, 0, 0};  // ids in the inputs, in the targets; runs
    HIPCHK(c, hipEventRecord(c->span_ev[0], s));
    if ((e = hipMemsetAsync(P.counters, 0, N_COUNTERS * 8, s)) != hipSuccess) return hip_fail("the counter reset", e);
    (void)hipEventRecord(c->span_ev[1], s);
    if (n_ids) {
        hipLaunchKernelGGL(k_span_flags, grid, block, 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_span_flags", e);
    }
    (void)hipEventRecord(c->span_ev[2], s);
    if (n_ids) {
        if (exclusive_scan<uint8_t>(s, P.start, n_ids, P.run, n_ids + 1) != 0) return hip_fail("the scan of the run starts", hipGetLastError());
        hipLaunchKernelGGL(k_span_place, grid, block, 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_span_place", e);
    }
    (void)hipEventRecord(c->span_ev[3], s);
    if (n_ids) {
        if (exclusive_scan<uint8_t>(s, P.c_in, n_ids, P.in_pos, n_ids + 1) != 0) return hip_fail("the scan of the input slots", hipGetLastError());
        if (exclusive_scan<uint8_t>(s, P.c_tgt, n_ids, P.tgt_pos, n_ids + 1) != 0) return hip_fail("the scan of the target slots", hipGetLastError());
        hipLaunchKernelGGL(k_span_offsets, dim3(cdiv64((uint64_t)n_docs + 1, SPAN_BLOCK)), block, 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_span_offsets", e);
        (void)hipMemcpyAsync(&h_tot[0], P.in_pos + n_ids, 8, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(&h_tot[1], P.tgt_pos + n_ids, 8, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(&h_tot[2], P.run + n_ids, 8, hipMemcpyDeviceToHost, s);
    } else {
        (void)hipMemsetAsync(c->span_in_off, 0, ((size_t)n_docs + 1) * 8, s);
        (void)hipMemsetAsync(c->span_tgt_off, 0, ((size_t)n_docs + 1) * 8, s);
    }
    (void)hipEventRecord(c->span_ev[4], s);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("the span passes", e);
    if (h_tot[0] > n_ids || h_tot[1] > 2 * n_ids + n_docs)  // (what the rule can give at most: the write pass stores by these)
        return hip_fail("the position scans", hipErrorUnknown);
    if (dmalloc(c, &c->span_in, h_tot[0]) != 0 || dmalloc(c, &c->span_tgt, h_tot[1]) != 0) {
        yabpe_span_free(c);
        return YABPE_E_HIP;
    }
    P.out_in = c->span_in;
    P.out_tgt = c->span_tgt;
    if (n_ids) {
        hipLaunchKernelGGL(k_span_write, grid, block, 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_span_write", e);
    }
    (void)hipEventRecord(c->span_ev[5], s);
    unsigned long long h_all[N_COUNTERS] = {0}, h_cnt[SPAN_COUNTERS] = {0, 0, 0, 0};
    (void)hipMemcpyAsync(h_all, P.counters, N_COUNTERS * 8, hipMemcpyDeviceToHost, s);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("k_span_write", e);
    for (uint32_t b = 0; b < MASK_SHARDS; ++b)
        for (uint32_t k = 0; k < SPAN_COUNTERS; ++k) h_cnt[k] += h_all[b * MASK_SHARD_STRIDE + k];
    float ms[5] = {0, 0, 0, 0, 0};
    auto &st = c->span_stats;
    st.total_ms = pass_times(c->span_ev, 5, ms);
    st.flags_ms = ms[1];
    st.index_ms = ms[2];
    st.place_ms = ms[3];
    st.write_ms = ms[4];
    st.kernel_ms = (double)ms[1] + ms[2] + ms[3] + ms[4];
    st.n_protected = h_cnt[SPAN_C_PROTECTED];
    st.n_noise = h_cnt[SPAN_C_NOISE];
    st.n_cut = h_cnt[SPAN_C_CUT];
    st.n_runs_over = h_cnt[SPAN_C_OVER];
    st.n_runs = h_tot[2];
    st.n_in = h_tot[0];
    st.n_tgt = h_tot[1];
    *out_dev_in = c->span_in;
    *out_dev_in_off = (uint64_t *)c->span_in_off;
    *out_n_in = h_tot[0];
    *out_dev_tgt = c->span_tgt;
    *out_dev_tgt_off = (uint64_t *)c->span_tgt_off;
    *out_n_tgt = h_tot[1];
    return YABPE_OK;
}

int yabpe_span_stats(yabpe_ctx *c, yabpe_span_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->span_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- fill-in-the-middle batches
namespace {
enum FimBuf { FB_PIECE_OFF = 0, FB_CUTS = 1, FB_IDS = 2, FB_LABELS = 3, FB_OFF = 4, FB_INFO = 5 };

void fim_free_bufs(yabpe_ctx *c, int first, int last) {
    for (int k = first; k <= last; ++k) {
        dfree(c->fim_buf[k]);
        c->fim_buf[k] = nullptr;
    }
}

// the checks both calls share: the rule's own, then the document starts -> *h_docs (n_docs entries; {0} without doc_off)
int fim_check(yabpe_ctx *c, const yabpe_fim_t *fim, const uint64_t *doc_off, uint32_t *n_docs, uint64_t limit, const char *what,
              std::vector<uint64_t> *h_docs) {
    if (!fim) return fail(c, YABPE_E_INVALID, "fim is NULL");
    static_assert(YABPE_FIM_EOT == FIM_EOT && YABPE_FIM_LOSS_MIDDLE == FIM_LOSS_MIDDLE && YABPE_FIM_PIECES == FIM_PIECES, "the header's and the rule's flags");
    if (!fim_rule_valid(fim->fim_threshold, fim->spm_threshold, fim->max_len, fim->flags))
        return fail(c, YABPE_E_INVALID, "fim_threshold %llu, spm_threshold %llu, max_len %llu, flags 0x%x: thresholds at most 2^32, max_len 0 or above %llu, flags within 0x%x",
                    (unsigned long long)fim->fim_threshold, (unsigned long long)fim->spm_threshold, (unsigned long long)fim->max_len, fim->flags,
                    fim_extra(fim->flags & FIM_FLAGS), FIM_FLAGS);
    if (!doc_off && *n_docs > 1) return fail(c, YABPE_E_INVALID, "doc_off is NULL with %u documents", *n_docs);
    if (!doc_off) *n_docs = 1;
    h_docs->assign(*n_docs, 0);
    if (doc_off && *n_docs) {
        if (is_device_ptr(doc_off)) HIPCHK(c, hipMemcpy(h_docs->data(), doc_off, (size_t)*n_docs * 8, hipMemcpyDeviceToHost));
        else memcpy(h_docs->data(), doc_off, (size_t)*n_docs * 8);
    }
    return check_starts(c, h_docs->data(), *n_docs, limit, what);
}
}  // namespace

int yabpe_fim_free(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    fim_free_bufs(c, FB_PIECE_OFF, FB_INFO);
    return YABPE_OK;
}

// BBPETokenizer.fim_cuts on the device (k_enc_lead_count, one scan, k_fim_cuts; the rule: fim_logic.h).  fim_ev[0..1] bracket
// the device work.  A call that the checks refuse has freed nothing.
int yabpe_fim_cuts(yabpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *doc_off, uint32_t n_docs, const yabpe_fim_t *fim,
                   uint64_t **out_dev_piece_off, uint64_t **out_dev_cuts) {
    if (!c || !out_dev_piece_off || !out_dev_cuts) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_piece_off = *out_dev_cuts = nullptr;
    if (n_bytes && !text) return fail(c, YABPE_E_INVALID, "text is NULL");
    std::vector<uint64_t> h_docs;
    TRY(fim_check(c, fim, doc_off, &n_docs, n_bytes, "text", &h_docs));
    fim_free_bufs(c, FB_PIECE_OFF, FB_CUTS);
    c->fim_stats = yabpe_fim_stats_t{};
    c->fim_stats.n_docs = n_docs;
    for (auto &e : c->fim_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    Scratch S(c->device, c->rank);
    FimCutParams P{};
    P.n_bytes = n_bytes;
    P.n_docs = n_docs;
    TRY(to_device(c, S, text, n_bytes, 16, &P.text));  // (enc_lead reads the text in aligned 16-byte chunks)
    TRY(to_device(c, S, (const unsigned long long *)h_docs.data(), (uint64_t)n_docs * 8, 8, &P.doc_off));
    const unsigned long long n_gran = (n_bytes + ENC_GRANULE - 1) / ENC_GRANULE;
    uint8_t *lead_cnt = nullptr;
    unsigned long long *table = nullptr, *piece_off = nullptr, *cuts = nullptr;
    HIPCHK(c, S.get(&lead_cnt, n_gran));
    HIPCHK(c, S.get(&table, n_gran + 1));
    TRY(dmalloc(c, &piece_off, 3ull * n_docs));
    c->fim_buf[FB_PIECE_OFF] = piece_off;
    TRY(dmalloc(c, &cuts, 3ull * n_docs));
    c->fim_buf[FB_CUTS] = cuts;
    P.table = table;
    P.seed = fim->seed;
    P.first_doc = fim->first_doc;
    P.fim = fim->fim_threshold;
    P.spm = fim->spm_threshold;
    P.piece_off = piece_off;
    P.cuts = cuts;
    auto hip_fail = [&](const char *what, hipError_t e) {
        (void)hipStreamSynchronize(s);
        fim_free_bufs(c, FB_PIECE_OFF, FB_CUTS);
        return fail(c, YABPE_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    HIPCHK(c, hipEventRecord(c->fim_ev[0], s));
    if (n_gran) {
        hipLaunchKernelGGL(k_enc_lead_count, dim3((uint32_t)((n_gran * 4 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, P.text, (unsigned long long)n_bytes, lead_cnt);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_enc_lead_count", e);
        if (exclusive_scan<uint8_t>(s, lead_cnt, n_gran, table, n_gran + 1) != 0) return hip_fail("the scan of the lead-byte counts", hipGetLastError());
    } else if ((e = hipMemsetAsync(table, 0, 8, s)) != hipSuccess) {
        return hip_fail("the table reset", e);
    }
    hipLaunchKernelGGL(k_fim_cuts, dim3(cdiv64(n_docs, FIM_BLOCK)), dim3(FIM_BLOCK), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_fim_cuts", e);
    (void)hipEventRecord(c->fim_ev[1], s);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("the cut passes", e);
    float ms[1] = {0};
    c->fim_stats.total_ms = pass_times(c->fim_ev, 1, ms);
    c->fim_stats.cuts_ms = ms[0];
    *out_dev_piece_off = (uint64_t *)piece_off;
    *out_dev_cuts = (uint64_t *)cuts;
    return YABPE_OK;
}

// BBPETokenizer.fim_tokens on the device (yabpe_fim_kernels.h; the rule: fim_logic.h).  fim_ev[0..3] bracket the call's device
// work: [1..2] the plan and the scan of the lengths, [2..3] the write.  The outputs are allocated after [2], once the total is
// on the host, so [2..3] holds that read-back and the allocation too.  A call that the checks refuse has freed nothing.
int yabpe_fim(yabpe_ctx *c, const uint32_t *ids, uint64_t n_ids, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *cuts,
              const yabpe_fim_t *fim, uint32_t **out_dev_ids, uint32_t **out_dev_labels, uint64_t **out_dev_off, uint32_t **out_dev_info,
              uint64_t *out_n_out) {
    if (!c || !out_dev_ids || !out_dev_labels || !out_dev_off || !out_dev_info || !out_n_out) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *out_dev_ids = *out_dev_labels = *out_dev_info = nullptr;
    *out_dev_off = nullptr;
    *out_n_out = 0;
    if (n_ids && !ids) return fail(c, YABPE_E_INVALID, "ids is NULL");
    const bool docs_dev = doc_off && is_device_ptr(doc_off);
    std::vector<uint64_t> h_docs;
    TRY(fim_check(c, fim, doc_off, &n_docs, n_ids, "ids", &h_docs));
    const bool pieces = (fim->flags & YABPE_FIM_PIECES) != 0;
    if (pieces && n_docs % 3 != 0) return fail(c, YABPE_E_INVALID, "%u documents with YABPE_FIM_PIECES: a multiple of 3 (prefix, middle, suffix)", n_docs);
    if (pieces && !cuts) return fail(c, YABPE_E_INVALID, "YABPE_FIM_PIECES needs the cuts of yabpe_fim_cuts");
    if (!pieces && cuts) return fail(c, YABPE_E_INVALID, "cuts are given without YABPE_FIM_PIECES");
    const uint32_t stride = pieces ? 3u : 1u, n_out_docs = n_docs / stride;
    for (uint32_t d = 0; d < n_out_docs; ++d) {
        const uint64_t last = (uint64_t)(d + 1) * stride < n_docs ? h_docs[(size_t)(d + 1) * stride] : n_ids;
        if (last - h_docs[(size_t)d * stride] > FIM_MAX_DOC)
            return fail(c, YABPE_E_CAPACITY, "document %u has %llu ids: at most 2^32 - 1", d, (unsigned long long)(last - h_docs[(size_t)d * stride]));
    }
    if (n_ids > LAY_MAX_SLOTS || n_ids + fim_extra(fim->flags) * n_out_docs > LAY_MAX_SLOTS)
        return fail(c, YABPE_E_CAPACITY, "%llu ids in %u documents: at most 2^36 output slots in one call", (unsigned long long)n_ids, n_out_docs);
    fim_free_bufs(c, FB_IDS, FB_INFO);
    const double cuts_ms = c->fim_stats.cuts_ms;
    c->fim_stats = yabpe_fim_stats_t{};
    c->fim_stats.cuts_ms = cuts_ms;
    c->fim_stats.n_docs = n_out_docs;
    for (auto &e : c->fim_ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    hipStream_t s = c->stream;
    Scratch S(c->device, c->rank);
    constexpr uint32_t N_COUNTERS = MASK_SHARDS * MASK_SHARD_STRIDE;
    FimParams P{};
    P.n_ids = n_ids;
    P.n_in = n_docs;
    P.n_docs = n_out_docs;
    TRY(to_device(c, S, ids, n_ids * 4, 4, &P.ids));
    TRY(to_device(c, S, docs_dev ? (const unsigned long long *)doc_off : (const unsigned long long *)h_docs.data(), (uint64_t)n_docs * 8, 8, &P.doc_off));
    if (pieces) TRY(to_device(c, S, (const unsigned long long *)cuts, (uint64_t)n_docs * 8, 8, &P.cuts));
    P.seed = fim->seed;
    P.first_doc = fim->first_doc;
    P.rule = FimRule{fim->fim_threshold, fim->spm_threshold, fim->pre_id, fim->suf_id, fim->mid_id, fim->eot_id, fim->ignore, fim->max_len, fim->flags};
    HIPCHK(c, S.get(&P.aux, n_out_docs));
    HIPCHK(c, S.get(&P.len, n_out_docs));
    HIPCHK(c, S.get(&P.counters, N_COUNTERS));
    unsigned long long *out_off = nullptr;
    uint4 *info = nullptr;
    TRY(dmalloc(c, &out_off, (uint64_t)n_out_docs + 1));
    c->fim_buf[FB_OFF] = out_off;
    TRY(dmalloc(c, &info, (uint64_t)n_out_docs));
    c->fim_buf[FB_INFO] = info;
    P.out_off = out_off;
    P.info = info;
    // the call fails: nothing of it is left in the context (the stream is drained first: Scratch hands its buffers back)
    auto hip_fail = [&](const char *what, hipError_t e) {
        (void)hipStreamSynchronize(s);
        fim_free_bufs(c, FB_IDS, FB_INFO);
        return fail(c, YABPE_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    unsigned long long h_out = 0;
    HIPCHK(c, hipEventRecord(c->fim_ev[0], s));
    if ((e = hipMemsetAsync(P.counters, 0, N_COUNTERS * 8, s)) != hipSuccess) return hip_fail("the counter reset", e);
    (void)hipEventRecord(c->fim_ev[1], s);
    if (n_out_docs) {
        hipLaunchKernelGGL(k_fim_plan, dim3(cdiv64(n_out_docs, FIM_BLOCK)), dim3(FIM_BLOCK), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_fim_plan", e);
        if (exclusive_scan<unsigned long long>(s, P.len, n_out_docs, out_off, (unsigned long long)n_out_docs + 1) != 0)
            return hip_fail("the scan of the sequence lengths", hipGetLastError());
        (void)hipMemcpyAsync(&h_out, out_off + n_out_docs, 8, hipMemcpyDeviceToHost, s);
    } else {
        (void)hipMemsetAsync(out_off, 0, 8, s);
    }
    (void)hipEventRecord(c->fim_ev[2], s);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("the plan pass", e);
    if (h_out > n_ids + fim_extra(fim->flags) * n_out_docs)  // (what the rule can give at most: the write pass stores by this)
        return hip_fail("the scan of the sequence lengths", hipErrorUnknown);
    uint32_t *o_ids = nullptr, *o_lab = nullptr;
    if (dmalloc(c, &o_ids, h_out) != 0 || dmalloc(c, &o_lab, h_out) != 0) {
        dfree(o_ids);
        fim_free_bufs(c, FB_IDS, FB_INFO);
        return YABPE_E_HIP;
    }
    c->fim_buf[FB_IDS] = o_ids;
    c->fim_buf[FB_LABELS] = o_lab;
    P.out_ids = o_ids;
    P.out_labels = o_lab;
    P.n_out = h_out;
    if (h_out) {
        hipLaunchKernelGGL(k_fim_write, dim3(cdiv64(h_out, FIM_BLOCK)), dim3(FIM_BLOCK), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail("k_fim_write", e);
    }
    (void)hipEventRecord(c->fim_ev[3], s);
    unsigned long long h_all[N_COUNTERS] = {0}, h_cnt[FIM_COUNTERS] = {0, 0, 0, 0};
    (void)hipMemcpyAsync(h_all, P.counters, N_COUNTERS * 8, hipMemcpyDeviceToHost, s);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail("k_fim_write", e);
    for (uint32_t b = 0; b < MASK_SHARDS; ++b)
        for (uint32_t k = 0; k < FIM_COUNTERS; ++k) h_cnt[k] += h_all[b * MASK_SHARD_STRIDE + k];
    float ms[3] = {0, 0, 0};
    auto &st = c->fim_stats;
    st.total_ms = pass_times(c->fim_ev, 3, ms);
    st.plan_ms = ms[1];
    st.write_ms = ms[2];
    st.n_psm = h_cnt[FIM_C_PSM];
    st.n_spm = h_cnt[FIM_C_SPM];
    st.n_truncated_docs = h_cnt[FIM_C_TRUNCATED];
    st.n_ids_dropped = h_cnt[FIM_C_DROPPED];
    st.n_out = h_out;
    *out_dev_ids = o_ids;
    *out_dev_labels = o_lab;
    *out_dev_off = (uint64_t *)out_off;
    *out_dev_info = (uint32_t *)info;
    *out_n_out = h_out;
    return YABPE_OK;
}

int yabpe_fim_stats(yabpe_ctx *c, yabpe_fim_stats_t *out) {
    if (!c || !out) return YABPE_E_INVALID;
    *out = c->fim_stats;
    return YABPE_OK;
}

// ---------------------------------------------------------------------------------------------- multi-GPU (see yabpe_comm.h)
int yabpe_comm_unique_id(uint8_t out_id[128]) {
    if (!out_id) return YABPE_E_INVALID;
    Rccl *R = rccl();
    if (!R) return fail(nullptr, YABPE_E_COMM, "librccl.so could not be loaded");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = R->GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, YABPE_E_COMM, "ncclGetUniqueId failed");
    memcpy(out_id, &id, 128);
    return YABPE_OK;
}

static int comm_attach(yabpe_ctx *c, int rank, int n_ranks) {
    if (c->have_words) return fail(c, YABPE_E_INVALID, "attach the communicator before yabpe_load_words");
    if (c->comm || c->ag_fn) return fail(c, YABPE_E_INVALID, "communicator already attached");
    if (c->id_bits == 32) return fail(c, YABPE_E_INVALID, "id_bits = 32 is single-device: no communicator can be attached");
    c->rank = rank;
    c->n_ranks = n_ranks;
    return 0;
}
static int comm_finish(yabpe_ctx *c) {
    TRY(dmalloc(c, &c->xsmall, 4 * (uint64_t)c->n_ranks));
    TRY(comm_buffers(c, (uint32_t)optv(c, "delta_cap", 16384)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return YABPE_OK;
}

int yabpe_comm_init(yabpe_ctx *c, int rank, int n_ranks, const uint8_t unique_id[128]) {
    if (!c || !unique_id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(comm_attach(c, rank, n_ranks));
    if (n_ranks == 1 && !optv(c, "force_comm", 0)) return YABPE_OK;
    c->multi = true;
    Rccl *R = rccl();
    if (!R) return fail(c, YABPE_E_COMM, "librccl.so could not be loaded");
    ncclUniqueId id;
    memcpy(&id, unique_id, 128);
    NCCLCHK(c, R->CommInitRank(&c->comm, n_ranks, id, rank));
    return comm_finish(c);
}

int yabpe_comm_enable_p2p(yabpe_ctx *c) {
    if (!c) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->multi) return YABPE_OK;  // one rank: nothing to exchange
    if (c->have_words) return fail(c, YABPE_E_INVALID, "enable the peer-to-peer exchange before yabpe_load_words");
    if (!c->p2p_e0) {
        HIPCHK(c, hipEventCreate(&c->p2p_e0));
        HIPCHK(c, hipEventCreate(&c->p2p_e1));
    }
    c->p2p = true;
    return p2p_setup(c);
}

int yabpe_comm_init_custom(yabpe_ctx *c, int rank, int n_ranks, yabpe_allgather_fn fn, void *user) {
    if (!c || !fn || n_ranks < 1 || rank < 0 || rank >= n_ranks) return YABPE_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(comm_attach(c, rank, n_ranks));
    if (n_ranks == 1 && !optv(c, "force_comm", 0)) return YABPE_OK;
    c->multi = true;
    c->ag_fn = fn;
    c->ag_user = user;
    return comm_finish(c);
}

}  // extern "C"
