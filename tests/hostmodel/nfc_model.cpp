// CPU model of yabpe_normalize: the rules of yet-another-bpe_amd/csrc/nfc_logic.h run in the steps the HIP kernels take
// (yabpe_norm_kernels.h) -- class pass per byte, the max-scan of the segment starts per 16-byte piece and per window of NFC_WIN
// bytes with the carry in front of every window, the dirty starts compacted, every dirty segment through a buffer of
// NFC_SHORT entries or, when it does not fit, through buffers sized from its measured length, the copy per window.  Test
// infrastructure only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../yet-another-bpe_amd/csrc/nfc_logic.h"
#include "../../yet-another-bpe_amd/csrc/unicode_norm.inc"

static std::vector<uint16_t> g_prop;
static std::vector<uint32_t> g_decomp, g_pairs;

static NfcTables tables() {
    if (g_prop.empty()) {
        g_prop.assign(0x110000, 0);
        for (unsigned r = 0; r < YB_NFC_PROP_NRUNS; ++r) {
            const unsigned lo = YB_NFC_PROP_RUNS[r][0], hi = r + 1 < YB_NFC_PROP_NRUNS ? YB_NFC_PROP_RUNS[r + 1][0] : 0x110000;
            for (unsigned cp = lo; cp < hi; ++cp) g_prop[cp] = (uint16_t)YB_NFC_PROP_RUNS[r][1];
        }
        for (unsigned r = 0; r < YB_NFC_NDECOMP; ++r)
            for (int k = 0; k < 5; ++k) g_decomp.push_back(YB_NFC_DECOMP[r][k]);
        for (unsigned r = 0; r < YB_NFC_NPAIRS; ++r)
            for (int k = 0; k < 3; ++k) g_pairs.push_back(YB_NFC_PAIRS[r][k]);
    }
    return NfcTables{g_prop.data(), g_decomp.data(), g_pairs.data(), YB_NFC_NDECOMP, YB_NFC_NPAIRS};
}

struct VecBuf {
    uint32_t *p;
    uint32_t get(uint32_t i) const { return p[i]; }
    void set(uint32_t i, uint32_t e) { p[i] = e; }
};

extern "C" const char *nfc_model_version() { return YB_NFC_UNIDATA_VERSION; }
extern "C" uint32_t nfc_model_prop(uint32_t cp) { return tables().prop[cp]; }
extern "C" int nfc_model_decompose(uint32_t cp, uint32_t *out) { return nfc_decompose(tables(), cp, out); }
extern "C" uint32_t nfc_model_compose(uint32_t a, uint32_t b) { return nfc_compose_pair(tables(), a, b); }
extern "C" uint32_t nfc_model_n_pairs() { return YB_NFC_NPAIRS; }
extern "C" void nfc_model_pair(uint32_t i, uint32_t *out) { memcpy(out, YB_NFC_PAIRS[i], 12); }
// 0 NFC_WIN, 1 NFC_PIECE, 2 NFC_SHORT, 3 NFC_CAP, 4 NFC_FIRST, 5 NFC_FIRST_DECOMP, 6 tile of the carry kernel (states per iteration)
extern "C" uint64_t nfc_model_const(int which) {
    const uint64_t v[] = {NFC_WIN, NFC_PIECE, NFC_SHORT, NFC_CAP, NFC_FIRST, NFC_FIRST_DECOMP, 256 * 8};
    return v[which];
}

// out: capacity 3 n + 1 bytes; out_off: n_parts + 1; stats: suspects, dirty segments, of them long, bytes copied (0: clean path).
// Returns 0, -7 (malformed UTF-8, *bad_pos = UnicodeDecodeError.start) or -4 (a dirty segment over NFC_CAP, *bad_pos = its start).
extern "C" int nfc_model(const uint8_t *text, uint64_t n, const uint64_t *part_off, uint32_t n_parts, uint8_t *out, uint64_t *out_off,
                         uint64_t *out_n, int64_t *bad_pos, uint64_t *stats) {
    const NfcTables T = tables();
    *bad_pos = -1;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    // ---- class pass
    std::vector<uint8_t> marks(n + 1, 0), meta(n + 1, 0);
    for (uint32_t p = 0; p < n_parts; ++p)
        if (part_off[p] < n) marks[part_off[p]] = NFC_PART0;
    const PtView v0{text, marks.data(), n, 0};
    for (uint64_t i = 0; i < n; ++i) {
        uint8_t m = NFC_START;
        if (text[i] & 0x80) {
            uint64_t end = n;
            for (uint64_t q = i + 1; q < i + 4 && q < n; ++q)
                if (marks[q] & NFC_PART0) {
                    end = q;
                    break;
                }
            bool bad = false;
            m = nfc_classify(v0, i, end, T, &bad);
            if (bad && *bad_pos < 0) *bad_pos = (int64_t)i;
            if (m & NFC_SUSPECT) ++stats[0];
        }
        meta[i] = m;
    }
    if (*bad_pos >= 0) return -7;
    for (uint32_t p = 0; p <= n_parts; ++p) out_off[p] = p < n_parts ? part_off[p] : n;
    *out_n = n;
    if (stats[0] == 0) {  // the clean path: the result is the input
        if (n) memcpy(out, text, n);
        return 0;
    }
    // ---- suspects -> dirty segment starts: windows, carry, apply
    const uint64_t n_win = (n + NFC_WIN - 1) / NFC_WIN, per_win = NFC_WIN / NFC_PIECE;
    auto piece = [&](uint64_t g) { return [&meta, g, n](int k) { return g + k < n ? meta[g + k] : (uint8_t)0; }; };
    std::vector<NfcPos> win(n_win, 0);
    for (uint64_t w = 0; w < n_win; ++w)
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * NFC_WIN + t * NFC_PIECE;
            win[w] = nfc_combine(win[w], nfc_piece_state(piece(g), g));
        }
    NfcPos run = 0;
    for (uint64_t w = 0; w < n_win; ++w) {
        const NfcPos mine = win[w];
        win[w] = run;
        run = nfc_combine(run, mine);
    }
    std::vector<uint8_t> flags(n, 0);
    for (uint64_t w = 0; w < n_win; ++w) {
        NfcPos before = win[w];
        for (uint64_t t = 0; t < per_win; ++t) {
            const uint64_t g = w * NFC_WIN + t * NFC_PIECE;
            nfc_piece_mark(before, piece(g), g, [&](uint64_t p) { flags[p] = 1; });
            before = nfc_combine(before, nfc_piece_state(piece(g), g));
        }
    }
    std::vector<unsigned long long> dstart;
    for (uint64_t i = 0; i < n; ++i)
        if (flags[i]) dstart.push_back(i);
    const uint64_t nd = dstart.size();
    stats[1] = nd;
    // ---- lengths: the short path, then the long one
    const PtView v{text, meta.data(), n, 0};
    std::vector<unsigned long long> dend(nd, 0), delta(nd, 0), shift(nd + 1, 0), long_list;
    std::vector<uint32_t> nent(nd, 0);
    uint32_t lane[NFC_SHORT];
    VecBuf sb{lane};
    for (uint64_t d = 0; d < nd; ++d) {
        const NfcSeg seg = nfc_seg_fill(T, v, dstart[d], sb, NFC_SHORT);
        dend[d] = seg.end;
        if (seg.in_cps > NFC_CAP) {
            if (*bad_pos < 0) *bad_pos = (int64_t)dstart[d];
            continue;
        }
        if (seg.n_ent > NFC_SHORT) {
            nent[d] = seg.n_ent;
            long_list.push_back(d);
            continue;
        }
        nfc_sort_insert(sb, 0, seg.n_ent);
        delta[d] = nfc_emit(sb, nfc_compose(T, sb, seg.n_ent), nullptr) - (seg.end - dstart[d]);
    }
    if (*bad_pos >= 0) return -4;
    stats[2] = long_list.size();
    std::vector<uint64_t> loff(nd + 1, 0);
    for (uint64_t d = 0; d < nd; ++d) loff[d + 1] = loff[d] + nent[d];
    std::vector<uint32_t> gbuf(loff[nd] + 1), gtmp(loff[nd] + 1);
    uint32_t cnt[256];
    auto long_pass = [&](bool write) {
        for (uint64_t d : long_list) {
            VecBuf b{gbuf.data() + loff[d]}, t{gtmp.data() + loff[d]};
            const NfcSeg seg = nfc_seg_fill(T, v, dstart[d], b, nent[d]);
            nfc_sort_long(b, t, seg.n_ent, cnt);
            const uint32_t m = nfc_compose(T, b, seg.n_ent);
            if (write) (void)nfc_emit(b, m, out + dstart[d] + shift[d]);
            else delta[d] = nfc_emit(b, m, nullptr) - (seg.end - dstart[d]);
        }
    };
    long_pass(false);
    for (uint64_t d = 0; d < nd; ++d) shift[d + 1] = shift[d] + delta[d];
    *out_n = n + shift[nd];
    // ---- write: copy per window and piece, the segments, the offsets
    for (uint64_t w = 0; w < n_win; ++w) {
        const uint64_t base = w * NFC_WIN, top = base + NFC_WIN < n ? base + NFC_WIN : n;
        const uint64_t klo = nfc_lower_bound(dstart.data(), 0, nd, base + 1), khi = nfc_lower_bound(dstart.data(), 0, nd, top);
        if (klo == khi && (klo == 0 || dend[klo - 1] <= base)) {
            for (uint64_t i = base; i < top; ++i) out[i + shift[klo]] = text[i];
            stats[3] += top - base;
            continue;
        }
        for (uint64_t g = base; g < top; g += NFC_PIECE) {
            uint64_t k = nfc_lower_bound(dstart.data(), klo, khi, g + 1);
            for (int j = 0; j < NFC_PIECE && g + j < top; ++j) {
                uint64_t dst = 0;
                if (nfc_copy_dst(dstart.data(), dend.data(), shift.data(), khi, g + j, &k, &dst)) {
                    out[dst] = text[g + j];
                    ++stats[3];
                }
            }
        }
    }
    for (uint64_t d = 0; d < nd; ++d) {
        if (nent[d]) continue;
        const NfcSeg seg = nfc_seg_fill(T, v, dstart[d], sb, NFC_SHORT);
        nfc_sort_insert(sb, 0, seg.n_ent);
        (void)nfc_emit(sb, nfc_compose(T, sb, seg.n_ent), out + dstart[d] + shift[d]);
    }
    long_pass(true);
    for (uint32_t p = 0; p < n_parts; ++p) out_off[p] = part_off[p] + shift[nfc_lower_bound(dstart.data(), 0, nd, part_off[p])];
    out_off[n_parts] = *out_n;
    return 0;
}
