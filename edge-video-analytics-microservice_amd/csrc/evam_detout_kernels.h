// evam_pp_detout_class / evam_pp_detout_merge: SSD DetectionOutput (the rule of evam_detout.h) on device memory.
// Included by evam_pp.hip inside its anonymous namespace's reach (kThreads, evam:: names).
#pragma once

namespace {

struct DetoutParams {
    const float* loc;     // [n][p][4]
    const float* conf;    // [n][p][c]
    const float* priors;  // [2][p][4]
    uint64_t* keys;       // scratch [n][c][top_k]: a class's kept keys, in its order
    uint32_t* kcount;     // scratch [n][c]: how many
    float* out;           // [n][keep_top_k][7]
    uint32_t* counts;     // [n] or NULL
    int n, p, c, bg, top_k, keep_top_k;
    float conf_thr, nms_thr;
};

// LDS every selection needs: a radix histogram, the per-wave counts of a chunk, two broadcast words.
struct DetoutSelLds {
    uint32_t hist[256];
    uint32_t w[2 * (kThreads / 64)];
    uint32_t bc[4];
};

// The M entries with the largest 32-bit keys of a sequence of n_seq entries, ties to the lower sequence index, handed
// to emit(position, index, key) with the positions in sequence order: an ordered compaction by ballots and prefix
// sums, with no atomic append. src(i, key) says whether entry i counts and gives its key (> 0). Returns how many were
// emitted, min(entries that count, M).
//
// When more than M count, the M-th largest key T is found by a radix select, 8 bits a pass from the top: a pass
// histograms one digit of the keys that share the digits found so far (LDS integer atomics: a count does not depend
// on the order of its increments), and a thread walks the 256 bins from the top to the bin that holds the M-th.
// Entries above T are all taken, and of those equal to T the first `need` in sequence order.
//
// Every barrier sits in a loop whose trip count depends on n_seq and on LDS words only: all threads take them alike.
template <class Src, class Emit>
__device__ inline uint32_t detout_select(DetoutSelLds& L, uint32_t n_seq, uint32_t M, const Src& src, const Emit& emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kThreads / 64;
    if (tid == 0) L.bc[0] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_seq; i += kThreads) {
        uint32_t key;
        mine += src(i, key) ? 1u : 0u;
    }
    if (mine) atomicAdd(&L.bc[0], mine);
    __syncthreads();
    const uint32_t total = L.bc[0];
    uint32_t T = 0, need = 0;
    if (total > M) {  // uniform
        uint32_t prefix = 0, remaining = M;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            L.hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < n_seq; i += kThreads) {
                uint32_t key;
                if (src(i, key) && (pass == 0 || (key >> (shift + 8)) == prefix)) atomicAdd(&L.hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t cum = 0;
                int d = 255;
                for (; d > 0; d--) {  // the bins hold at least `remaining` together: the walk ends at d >= 0
                    if (cum + L.hist[d] >= remaining) break;
                    cum += L.hist[d];
                }
                L.bc[1] = (uint32_t)d;
                L.bc[2] = remaining - cum;
            }
            __syncthreads();
            prefix = (prefix << 8) | L.bc[1];
            remaining = L.bc[2];
        }
        T = prefix;
        need = remaining;
    }
    static_assert(kThreads == 256, "hist is zeroed one word a thread");
    uint32_t gt_total = 0, eq_total = 0;
    for (uint32_t i0 = 0; i0 < n_seq; i0 += kThreads) {
        const uint32_t i = i0 + (uint32_t)tid;
        uint32_t key = 0;
        const bool ok = i < n_seq && src(i, key);
        const bool gt = ok && key > T, eq = ok && key == T && need > 0;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        if (lane == 0) {
            L.w[wave] = (uint32_t)__popcll(mg);
            L.w[kWaves + wave] = (uint32_t)__popcll(me);
        }
        __syncthreads();
        uint32_t g_before = 0, g_all = 0, e_before = 0, e_all = 0;
        for (int v = 0; v < kWaves; v++) {
            g_before += v < wave ? L.w[v] : 0u;
            g_all += L.w[v];
            e_before += v < wave ? L.w[kWaves + v] : 0u;
            e_all += L.w[kWaves + v];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const uint32_t g_rank = gt_total + g_before + (uint32_t)__popcll(mg & below);
        const uint32_t e_rank = eq_total + e_before + (uint32_t)__popcll(me & below);
        if (gt || (eq && e_rank < need)) emit(g_rank + (e_rank < need ? e_rank : need), i, key);
        gt_total += g_all;
        eq_total += e_all;
        __syncthreads();  // L.w is rewritten by the next chunk
    }
    return total < M ? total : M;
}

// One workgroup per (class, image): steps 1 to 4 of the rule. The class's candidates are selected straight from conf
// (no scratch of P entries), sorted in LDS by their 64-bit keys (bitonic, the keys are distinct), decoded into LDS and
// walked in order; each is tested against the kept list by all threads at once and the flags are reduced by the
// barrier. The kept keys go to scratch in their order, which is what the merge needs.
__global__ __launch_bounds__(kThreads) void evam_pp_detout_class(const DetoutParams P) {
    __shared__ uint64_t s_keys[kDetoutMaxTopK];
    __shared__ DetBox s_box[kDetoutMaxTopK];
    __shared__ uint16_t s_kept[kDetoutMaxTopK];
    __shared__ uint8_t s_ok[kDetoutMaxTopK];
    __shared__ DetoutSelLds L;
    static_assert(kDetoutMaxTopK <= 65536, "s_kept holds positions");

    const int tid = threadIdx.x;
    const int c = blockIdx.x, n = blockIdx.y;
    uint32_t* kc = P.kcount + (size_t)n * P.c + c;
    if (c == P.bg) {  // uniform
        if (tid == 0) *kc = 0;
        return;
    }
    const float* conf = P.conf + (size_t)n * P.p * P.c + c;
    const int C = P.c;
    const float thr = P.conf_thr;
    const uint32_t top_k = (uint32_t)P.top_k;  // <= kDetoutMaxTopK (checked by the host)
    const auto src = [=](uint32_t i, uint32_t& key) {
        const float s = conf[(size_t)i * C];
        key = detout_bits(s);
        return detout_candidate(s, thr);
    };
    const auto emit = [&](uint32_t pos, uint32_t i, uint32_t key) {
        if (pos < (uint32_t)kDetoutMaxTopK) s_keys[pos] = ((uint64_t)key << 32) | (uint32_t)~i;
    };
    const int m = (int)detout_select(L, (uint32_t)P.p, top_k, src, emit);

    int n2 = 1;
    while (n2 < m) n2 <<= 1;  // <= kDetoutMaxTopK
    for (int i = m + tid; i < n2; i += kThreads) s_keys[i] = 0;  // below every key
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t a = s_keys[i], b = s_keys[l];
                    if ((i & k) == 0 ? a < b : a > b) {  // descending
                        s_keys[i] = b;
                        s_keys[l] = a;
                    }
                }
            }
            __syncthreads();
        }

    const float* var = P.priors + (size_t)P.p * 4;
    const float* loc = P.loc + (size_t)n * P.p * 4;
    for (int j = tid; j < m; j += kThreads) {
        const size_t p = detout_key_p(s_keys[j]);  // < P.p: the key was built from an index below it
        DetBox b;
        s_ok[j] = detout_decode(P.priors + p * 4, var + p * 4, loc + p * 4, b) ? 1 : 0;
        s_box[j] = b;
    }
    __syncthreads();

    int nk = 0;  // uniform
    const float nms = P.nms_thr;
    for (int i = 0; i < m; i++) {
        if (!s_ok[i]) continue;  // the same LDS byte for every thread
        const DetBox it = s_box[i];
        int drop = 0;
        for (int k = tid; k < nk; k += kThreads) drop |= detout_suppresses(it, s_box[s_kept[k]], nms) ? 1 : 0;
        if (__syncthreads_or(drop)) continue;
        if (tid == 0) s_kept[nk] = (uint16_t)i;
        nk++;
        __syncthreads();  // the next candidate reads the new entry
    }
    uint64_t* gk = P.keys + ((size_t)n * P.c + c) * (size_t)P.top_k;
    for (int k = tid; k < nk; k += kThreads) gk[k] = s_keys[s_kept[k]];  // nk <= m <= top_k
    if (tid == 0) *kc = (uint32_t)nk;
}

// One workgroup per image: steps 5 and 6. The sequence is the kept keys of the image's classes, class-major and in
// each class's order, so "ties to the lower sequence index" is "lower class, then lower p", and the sequence order of
// the survivors is the order of the rows: the ordered compaction leaves nothing to sort.
__global__ __launch_bounds__(kThreads) void evam_pp_detout_merge(const DetoutParams P) {
    __shared__ uint64_t s_keys[kDetoutMaxTopK];
    __shared__ uint16_t s_cls[kDetoutMaxTopK];
    __shared__ uint32_t s_cnt[kDetoutMaxClasses];
    __shared__ DetoutSelLds L;

    const int tid = threadIdx.x;
    const int n = blockIdx.x;
    const uint32_t top_k = (uint32_t)P.top_k;
    for (int c = tid; c < P.c; c += kThreads) {
        const uint32_t v = P.kcount[(size_t)n * P.c + c];
        s_cnt[c] = v < top_k ? v : top_k;
    }
    __syncthreads();
    const uint64_t* gk = P.keys + (size_t)n * P.c * (size_t)top_k;
    const uint32_t K = (uint32_t)P.keep_top_k;  // <= kDetoutMaxTopK
    const auto src = [&](uint32_t i, uint32_t& key) {
        const uint32_t c = i / top_k, j = i - c * top_k;
        if (j >= s_cnt[c]) return false;
        key = (uint32_t)(gk[i] >> 32);
        return true;
    };
    const auto emit = [&](uint32_t pos, uint32_t i, uint32_t) {
        if (pos < (uint32_t)kDetoutMaxTopK) {
            s_keys[pos] = gk[i];
            s_cls[pos] = (uint16_t)(i / top_k);
        }
    };
    const uint32_t m = detout_select(L, (uint32_t)P.c * top_k, K, src, emit);
    __syncthreads();

    const float* var = P.priors + (size_t)P.p * 4;
    const float* loc = P.loc + (size_t)n * P.p * 4;
    float* out = P.out + (size_t)n * K * 7;
    for (uint32_t r = tid; r < K; r += kThreads) {
        float* row = out + (size_t)r * 7;
        if (r < m) {
            const uint64_t key = s_keys[r];
            const size_t p = detout_key_p(key);
            DetBox b;
            (void)detout_decode(P.priors + p * 4, var + p * 4, loc + p * 4, b);  // finite: the class kernel kept it
            detout_row(row, n, (int)s_cls[r], key, b);
        } else {
            detout_fill_row(row);
        }
    }
    if (tid == 0 && P.counts) P.counts[n] = m;
}

}  // namespace
