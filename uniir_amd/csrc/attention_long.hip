// Fused attention for sequences of 513 .. 1024 tokens (head_dim 64).  Three families of kernels on the same bodies:
//   attn_long_*  : plain self-attention (no causal mask, no bias, no dropout, dense rows), forward in bf16 / fp16 and backward in
//                  bf16.  CLIP ViT-L/14@336px: 577 tokens.
//   attn_xlong_* : the general form (Q separate from K | V, uniir_attention_fwd_long / _bwd_long) in bf16: per-item key counts
//                  (key_len), packed query rows (q_row_off) and probability dropout (DROP).  BLIP MED cross-attention over the
//                  577 image tokens of a 384-pixel ViT.  Every size from 1 x 1 to 1024 x 1024 runs here.
//   attn_rlong_* : T5-style self-attention on the packed [q | k | v] buffer (uniir_attention_rel_fwd_long / _rel_bwd_long) in bf16,
//                  the forward without dropout in fp16 too (uniir_attn_rel_fwd_long_f16):
//                  logits = scale * q.k + rel_emb[rel_bucket[key - query + seq - 1]][head] (REL), scale a run-time argument,
//                  probability dropout, the bias gradient drel in a fixed order.  CLIP_FF at ViT-L/14@336px: 577 + 77 = 654 fused tokens.
//
// A head of that length no longer fits LDS whole (attention.hip: 2 * 512 * 128 bytes), so one operand is STREAMED: a workgroup
// (8 waves) owns 128 rows of one (item, head) -- every wave one 16-row tile for the whole sweep, its accumulators in registers --
// and the other side passes through LDS in chunks, double-buffered ([row][64] 16-bit, the swizzled image and the fragment
// helpers of attention.h).  The next chunk is fetched into registers before the current one is computed and written to the
// other buffer behind it (register staging; one barrier per chunk).
//   forward : owns 128 queries, streams K / V in 128-key chunks; online softmax with the per-row deferred maximum of attn_fwd_kernel
//   dK / dV : owns 128 keys, streams Q / dO (and the per-row lse, delta) in query chunks
//   dQ      : owns 128 queries, streams K / V in key chunks
// The backward is the two phases of attn_bwd_kernel as two kernels; neither sums across workgroups, nothing is atomic, every sum
// has a fixed order: the results are bitwise reproducible.  delta = rowsum(dO . O) is recomputed from the O / dO rows (the ABI has no
// workspace): 8 lanes hold a row's 16-byte pieces, their partial dots meet in a fixed butterfly.
// A query row's result never depends on the rows that share its tile or its workgroup (the rescale decision is per row).
// The bodies are templates: XL = per-item ranges (the queries of item m are rows row_off[m] .. of q / out / dout / dq, its keys stop at
// kvalid = min(Tk, klen[m]); lse and the dropout coordinates keep the dense [item][head][a.Tq] x a.Tk numbering), DROP = dropout of
// P.  The attn_long_* kernels are the <XL = false, DROP = false> instantiations.
// REL (with XL = false, Tq == Tk): the bias of every diagonal key - query sits in LDS, premultiplied by log2 e and filled once per
// workgroup: the forward and dQ hold the whole table (2 seq - 1 floats, indexed key + (Tq - 1 - query) with the streamed chunk's
// first key k0 inside `key`), dK / dV the 128 + seq - 1 diagonals its 128 keys see (indexed (key - first key) + Tq - 1 - query with
// the streamed chunk's first row r0 inside `query`).  Both tables carry 32 zero slots of slack where the dead rows / keys of a last
// block point, so no index is clamped.  dK / dV also sums dS along the diagonals for drel (the scheme of attn_bwd_kernel).
#include "attention.h"

#define AL_THREADS 512
#define AL_WAVES (AL_THREADS / 64)
#define AL_ROWS (16 * AL_WAVES)      // rows a workgroup owns
#define AL_KV 128                    // K / V rows per streamed chunk (forward, dQ)
#define AL_QC 64                     // Q / dO rows per streamed chunk (dK / dV: three operands ride the registers there)

// the 16-byte pieces of rows r0 .. r0 + CH - 1 of a [T][64] head slice: piece c = u * AL_THREADS + tid is row c / 8, columns 8 (c % 8) ..
// (loads come from clamped, always valid rows; rows >= T are zeroed at the LDS store)
template <int CH>
DEVINL void al_load(u32x4_t (&v)[CH * 8 / AL_THREADS], const unsigned short* __restrict__ src, long ld, int r0, int T, int tid) {
#pragma unroll
    for (int u = 0; u < CH * 8 / AL_THREADS; ++u) {
        const int c = u * AL_THREADS + tid;
        const int row = min(r0 + (c >> 3), T - 1), kc = c & 7;
        v[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(src + (long)row * ld + kc * 8));
    }
}
template <int CH>
DEVINL void al_store(char* lds, const u32x4_t (&v)[CH * 8 / AL_THREADS], int r0, int T, int tid) {
#pragma unroll
    for (int u = 0; u < CH * 8 / AL_THREADS; ++u) {
        const int c = u * AL_THREADS + tid;
        const int row = c >> 3, kc = c & 7;
        const u32x4_t z = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4_t*>(lds + row * 128 + ((kc ^ (row & 7)) << 4)) = (r0 + row < T) ? v[u] : z;
    }
}
// delta of the rows whose O / dO pieces the workgroup holds: dl[row] = dO[row] . O[row] (0 for rows >= T).  The 8 lanes of a row are
// neighbours; the butterfly leaves the same sum in all of them.
template <int CH>
DEVINL void al_delta(float* dl, const u32x4_t (&o)[CH * 8 / AL_THREADS], const u32x4_t (&d)[CH * 8 / AL_THREADS], int r0, int T, int tid) {
#pragma unroll
    for (int u = 0; u < CH * 8 / AL_THREADS; ++u) {
        const int c = u * AL_THREADS + tid;
        const int row = c >> 3, kc = c & 7;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s += __uint_as_float(o[u][e] << 16) * __uint_as_float(d[u][e] << 16);
            s += __uint_as_float(o[u][e] & 0xffff0000u) * __uint_as_float(d[u][e] & 0xffff0000u);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (kc == 0) dl[row] = (r0 + row < T) ? s : 0.f;
    }
}

// REL: tab[j] = rel_emb[rel_bucket[d0 + j]][h] * log2 e for the diagonals d0 + j in [0, nd), zero for the other slots of tab[0 .. n)
DEVINL void al_fill_bias(float* tab, const AttnArgs& a, int h, int d0, int nd, int n, int tid) {
    for (int j = tid; j < n; j += AL_THREADS) {
        const int d = d0 + j;
        tab[j] = (d >= 0 && d < nd) ? a.rel_emb[a.rel_bucket[d] * a.H + h] * LOG2EF : 0.f;
    }
}

// ---------------- forward ----------------
// the rows of item m: first query row and query count (packed with XL and row_off), the keys a sweep visits
template <bool XL>
DEVINL void al_item(const AttnArgs& a, int m, long& qr0, int& Tq, int& kvalid) {
    Tq = a.Tq;
    qr0 = (long)m * Tq;
    kvalid = a.Tk;
    if (XL) {
        if (a.row_off) {
            qr0 = a.row_off[m];
            Tq = a.row_off[m + 1] - a.row_off[m];
        }
        if (a.klen) kvalid = min(a.Tk, a.klen[m]);
    }
}

template <bool F16, bool XL, bool DROP, bool REL = false>
DEVINL void al_fwd_body(const AttnArgs& a, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int NL = AL_KV * 8 / AL_THREADS;
    constexpr int BUF = 2 * AL_KV * 128;      // K chunk, V chunk
    const int H = a.H;
    const int qb = blockIdx.x % nqb, mh = blockIdx.x / nqb;      // the query blocks of a head are neighbours: K / V stay in L2
    const int m = mh / H, h = mh % H;
    long qr0;
    int Tq, Tk;          // Tk: the keys of the sweep (XL: the item's valid keys; the masked ones are never staged)
    al_item<XL>(a, m, qr0, Tq, Tk);
    if (XL && qb * AL_ROWS >= Tq) return;      // a packed item shorter than the call's tq (the whole workgroup leaves)
    long kr0 = (long)m * a.Tk;
    if (XL && a.kv_row_off) {      // the forward alone (uniir_onequery_fwd): the item's keys are its own packed rows, its length the key count
        kr0 = a.kv_row_off[m];
        Tk = min(Tk, a.kv_row_off[m + 1] - a.kv_row_off[m]);
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned short* qbase = a.q + qr0 * a.q_ld + h * ATT_D;
    const unsigned short* kbase = a.k + kr0 * a.kv_ld + h * ATT_D;
    const unsigned short* vbase = a.v + kr0 * a.kv_ld + h * ATT_D;
    const unsigned dth = DROP ? drop_threshold(a.drop_p) : 0u;
    const float dks = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const int qi = lane & 15, g = lane >> 4;
    const int q0 = qb * AL_ROWS + w * 16, q = q0 + qi;
    const bool active = q0 < Tq;          // wave-uniform; an idle wave still stages and meets the barriers
    const float sl2 = REL ? a.scale * LOG2EF : SCALE_LOG2E;
    const float es = REL ? 1.0f : sl2;          // REL: the scale goes in with the bias, the logits are in log2 units from there on
    const float* dbias = reinterpret_cast<const float*>(lds + 2 * BUF) + (Tq - 1 - min(q, Tq - 1));      // + key: the lane's row of the bias
    if (REL) al_fill_bias(reinterpret_cast<float*>(lds + 2 * BUF), a, h, 0, Tq + Tk - 1, Tq + Tk + 31, tid);
    bf16x8_t qf[2];
    qf[0] = frag_rows_global(qbase, a.q_ld, q0, 0, lane, Tq);
    qf[1] = frag_rows_global(qbase, a.q_ld, q0, 1, lane, Tq);
    u32x4_t rk[NL], rv[NL];
    al_load<AL_KV>(rk, kbase, a.kv_ld, 0, Tk, tid);
    al_load<AL_KV>(rv, vbase, a.kv_ld, 0, Tk, tid);
    al_store<AL_KV>(lds, rk, 0, Tk, tid);
    al_store<AL_KV>(lds + AL_KV * 128, rv, 0, Tk, tid);
    __syncthreads();
    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f;
    f32x4_t l4 = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int nch = (Tk + AL_KV - 1) / AL_KV;
    for (int c = 0; c < nch; ++c) {
        const char* ldsK = lds + (c & 1) * BUF;
        const char* ldsV = ldsK + AL_KV * 128;
        const int k0 = c * AL_KV;
        if (c + 1 < nch) {
            al_load<AL_KV>(rk, kbase, a.kv_ld, k0 + AL_KV, Tk, tid);
            al_load<AL_KV>(rv, vbase, a.kv_ld, k0 + AL_KV, Tk, tid);
        }
        if (active) {
            const int nkb = min(AL_KV / 32, (Tk - k0 + 31) >> 5);      // >= 1
            // the block structure of attn_fwd_kernel: S^T of a 32-key block one block ahead of its softmax, two logit buffers
            auto s_block = [&](int kb, f32x4_t (&sx)[2]) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    sx[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 2; ++s) sx[kt] = mfma16x<F16>(frag_rows(ldsK, kb * 32 + kt * 16, s, lane), qf[s], sx[kt]);
                }
            };
            auto softmax_pv = [&](int kb, f32x4_t (&st)[2]) {
                if (REL) {
                    const float* bp = dbias + k0 + kb * 32 + 4 * g;
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[kt][r] = __builtin_fmaf(st[kt][r], sl2, bp[kt * 16 + r]);
                }
                if (k0 + kb * 32 + 32 > Tk) {
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + kb * 32 + kt * 16 + 4 * g + r >= Tk) st[kt][r] = -1e30f;
                }
                // deferred maximum, decided per row (see attn_fwd_kernel): the reference moves when one of the row's own logits
                // exceeds it by more than ATT_DEFER; alpha is exactly 1 for the rows that keep theirs
                float mx = -1e30f;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[kt][r]);
                const unsigned long long over = __ballot(__builtin_fmaf(mx, es, -m_run) > ATT_DEFER);
                unsigned rows_over = (unsigned)(over | (over >> 32));
                rows_over = (rows_over | (rows_over >> 16)) & 0xffffu;
                if (rows_over) {
                    const float gm = group_max(mx);
                    const float m_new = ((rows_over >> qi) & 1u) ? fmaxf(m_run, gm * es) : m_run;
                    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                    l4 = l4 * alpha;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) o[dt] = o[dt] * alpha;
                    m_run = m_new;
                }
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const f32x4_t arg = __builtin_elementwise_fma(st[kt], f32x4_t{es, es, es, es}, f32x4_t{-m_run, -m_run, -m_run, -m_run});
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[kt][r] = __builtin_amdgcn_exp2f(arg[r]);
                    l4 = l4 + st[kt];
                }
                if (DROP) {      // acc[r] = S[key = 4g + r][q = qi]; dense coordinates: packed rows draw the dense call's mask
                    const unsigned rowbase = (unsigned)((((long)m * H + h) * a.drop_tq + a.drop_q0 + q) * a.Tk);
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            st[kt][r] *= drop_scale(rowbase + (unsigned)(k0 + kb * 32 + kt * 16 + 4 * g + r), a.drop_seed, dth, dks);
                }
                const bf16x8_t pf = pack8x<F16>(st[0], st[1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = mfma16x<F16>(frag_cols_tr(ldsV, kb * 32, dt, lane), pf, o[dt]);
            };
            f32x4_t sa[2], sb[2];
            s_block(0, sa);
            for (int kb = 0; kb < nkb; kb += 2) {
                if (kb + 1 < nkb) s_block(kb + 1, sb);
                softmax_pv(kb, sa);
                if (kb + 1 >= nkb) break;
                if (kb + 2 < nkb) s_block(kb + 2, sa);
                softmax_pv(kb + 1, sb);
            }
        }
        if (c + 1 < nch) {
            char* nx = lds + ((c + 1) & 1) * BUF;      // last read in iteration c - 1, which every wave has left (barrier below)
            al_store<AL_KV>(nx, rk, k0 + AL_KV, Tk, tid);
            al_store<AL_KV>(nx + AL_KV * 128, rv, k0 + AL_KV, Tk, tid);
        }
        __syncthreads();
    }
    if (active) {
        const float l_run = group_sum((l4[0] + l4[1]) + (l4[2] + l4[3]));
        const bool live = q < Tq;
        att_store_tile<F16>(o, 1.0f / l_run, a.out + (qr0 + min(q, Tq - 1)) * a.out_ld + h * ATT_D, live, g);
        if (live && g == 0) a.lse[((long)m * H + h) * a.Tq + q] = m_run * LN2F + __logf(l_run);
    }
}
template <bool F16>
__global__ __launch_bounds__(AL_THREADS) void attn_long_fwd_kernel(AttnArgs a, int nqb) {
    al_fwd_body<F16, false, false>(a, nqb);
}
template <bool DROP, bool F16 = false>
__global__ __launch_bounds__(AL_THREADS) void attn_xlong_fwd_kernel(AttnArgs a, int nqb) {
    al_fwd_body<F16, true, DROP>(a, nqb);
}
template <bool DROP, bool F16 = false>
__global__ __launch_bounds__(AL_THREADS, 4) void attn_rlong_fwd_kernel(AttnArgs a, int nqb) {
    al_fwd_body<F16, false, DROP, true>(a, nqb);
}

// the lane parts of the swizzled fragment addresses (attn_bwd_kernel): row fragments of k-step s, transposed fragments of column tile dt
struct AlOffs {
    int r[2], t[4];
};
DEVINL AlOffs al_offs(int li, int g) {
    AlOffs x;
#pragma unroll
    for (int s = 0; s < 2; ++s) x.r[s] = li * 128 + (((s * 4 + g) ^ (li & 7)) << 4);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int row = 4 * g + (li >> 2), col = 16 * dt + 4 * (li & 3);
        x.t[dt] = row * 128 + ((((col >> 3) ^ (row & 7)) << 4) | ((col & 7) << 1));
    }
    return x;
}
DEVINL bf16x8_t al_rows_frag(const char* p) { return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(p)); }
DEVINL bf16x8_t al_cols_frag(const char* p) {      // 32-row block: rows 4g.., 16 + 4g.. of one column tile
    const u32x2_t l2 = __builtin_bit_cast(u32x2_t, lds_read_tr16(p));
    const u32x2_t h2 = __builtin_bit_cast(u32x2_t, lds_read_tr16(p + 2048));
    const u32x4_t r = {l2[0], l2[1], h2[0], h2[1]};
    return __builtin_bit_cast(bf16x8_t, r);
}

// ---------------- backward: dK, dV (phase 1 of attn_bwd_kernel, the queries streamed) ----------------
// buffer: Q chunk, dO chunk, lse * log2 e, delta.  Rows >= Tq of a chunk are zero in all four: p = 1, dP = 0, dS = 0, and the zero dO / Q
// rows add nothing.  A key's dK / dV column depends on that key alone, so the dead keys of the last tile need no mask: they are not stored.
// XL: the key rows kvalid .. Tk - 1 of an item are masked: their dK / dV rows are written as exact zeros (a tile behind kvalid skips the
// sweep; in the tile that holds the edge a lane's accumulators belong to its own key alone and are cleared before the store).
// REL: behind the two buffers sit bsum [64] (the bucket sums) and ddiag [Tq + 164] (the diagonal sums), both 64-bit fixed point
// (att_drel_fix), and dbias [Tq + 164].  Slot j of ddiag / dbias is the diagonal (first key of the workgroup) + j - 36: the element
// (key, query) has j = (key - first key) + Tq + 35 - query, 5 <= j <= Tq + 162 over every row and key a block can hold, dead ones
// included (the pre-summed value of a lane goes three slots lower: >= 2); the live elements (key < Tk, query < Tq) fill 36 .. 162 + Tq.  Dead rows get p = 0 (their Q / dO / lse / delta are zero, but
// exp2 of a bias alone need not be 1), and dead rows and keys add nothing to ddiag.
template <bool XL, bool DROP, bool REL = false>
DEVINL void al_dkdv_body(const AttnArgs& a, int nkblk) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int NL = AL_QC * 8 / AL_THREADS;
    constexpr int BUF = 2 * AL_QC * 128 + 2 * AL_QC * 4;
    const int H = a.H, Tk = a.Tk;
    const int kblk = blockIdx.x % nkblk, mh = blockIdx.x / nkblk;
    const int m = mh / H, h = mh % H;
    long qr0;
    int Tq, kvalid;
    al_item<XL>(a, m, qr0, Tq, kvalid);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned short* qbase = a.q + qr0 * a.q_ld + h * ATT_D;
    const unsigned short* kbase = a.k + (long)m * Tk * a.kv_ld + h * ATT_D;
    const unsigned short* vbase = a.v + (long)m * Tk * a.kv_ld + h * ATT_D;
    const unsigned short* obase = a.out + qr0 * a.out_ld + h * ATT_D;
    const unsigned short* dobase = a.dout + qr0 * a.out_ld + h * ATT_D;
    const float* lsebase = a.lse + ((long)m * H + h) * a.Tq;
    const unsigned dth = DROP ? drop_threshold(a.drop_p) : 0u;
    const float dks = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const unsigned headbase = (unsigned)((((long)m * H + h) * a.drop_tq + a.drop_q0) * a.Tk);      // dense coordinates (see the forward)
    const int li = lane & 15, g = lane >> 4;
    const int k0 = kblk * AL_ROWS + w * 16, key = k0 + li;
    const float sl2 = REL ? a.scale * LOG2EF : SCALE_LOG2E;
    const float oscale = REL ? a.scale : ATT_SCALE;
    unsigned long long* bsum = reinterpret_cast<unsigned long long*>(lds + 2 * BUF);
    unsigned long long* ddiag = bsum + 64;
    const int nslot = Tq + 164;
    float* dbias = reinterpret_cast<float*>(ddiag + nslot);
    const int jl = w * 16 + li + Tq + 35;          // - query: the lane's slot
    if (REL) {
        al_fill_bias(dbias, a, h, kblk * AL_ROWS - 36, Tq + Tk - 1, nslot, tid);
        if (tid < 64) bsum[tid] = 0ull;
        for (int j = tid; j < nslot; j += AL_THREADS) ddiag[j] = 0ull;
    }
    const bool stores = k0 < Tk;                                  // wave-uniform
    const bool active = XL ? k0 < kvalid : stores;                // the waves that run the sweep; the others only stage
    const int nch = (XL && kblk * AL_ROWS >= kvalid) ? 0 : (Tq + AL_QC - 1) / AL_QC;      // a workgroup of masked keys streams nothing
    bf16x8_t kf[2], vf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        kf[s] = frag_rows_global(kbase, a.kv_ld, k0, s, lane, Tk);
        vf[s] = frag_rows_global(vbase, a.kv_ld, k0, s, lane, Tk);
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t dv[4], dk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        dv[dt] = zero4;
        dk[dt] = zero4;
    }
    const AlOffs off = al_offs(li, g);
    u32x4_t rq[NL], rdo[NL], ro[NL];
    float rl = 0.f;
    auto fetch = [&](int r0) {
        al_load<AL_QC>(rq, qbase, a.q_ld, r0, Tq, tid);
        al_load<AL_QC>(rdo, dobase, a.out_ld, r0, Tq, tid);
        al_load<AL_QC>(ro, obase, a.out_ld, r0, Tq, tid);
        if (tid < AL_QC) rl = lsebase[min(r0 + tid, Tq - 1)];
    };
    auto put = [&](char* buf, int r0) {
        al_store<AL_QC>(buf, rq, r0, Tq, tid);
        al_store<AL_QC>(buf + AL_QC * 128, rdo, r0, Tq, tid);
        float* st = reinterpret_cast<float*>(buf + 2 * AL_QC * 128);
        if (tid < AL_QC) st[tid] = (r0 + tid < Tq) ? rl * LOG2EF : 0.f;
        al_delta<AL_QC>(st + AL_QC, ro, rdo, r0, Tq, tid);
    };
    if (!XL || nch > 0) {
        fetch(0);
        put(lds, 0);
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const char* bufA = lds + (c & 1) * BUF;      // Q; dO sits AL_QC * 128 bytes behind it at the same lane offsets
        constexpr int dAB = AL_QC * 128;
        const float* lse2 = reinterpret_cast<const float*>(bufA + 2 * AL_QC * 128);
        const float* Dq = lse2 + AL_QC;
        const int r0 = c * AL_QC;
        if (c + 1 < nch) fetch(r0 + AL_QC);
        if (active) {
            const int nqblk = min(AL_QC / 32, (Tq - r0 + 31) >> 5);
            for (int qb = 0; qb < nqblk; ++qb) {
                const int blk = qb * 4096;
                const bool qedge = REL && r0 + qb * 32 + 32 > Tq;
                f32x4_t pt[2], dst[2];
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    f32x4_t sa = zero4, dp = zero4;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        sa = mfma16(al_rows_frag(bufA + off.r[s] + blk + qt * 2048), kf[s], sa);
                        dp = mfma16(al_rows_frag(bufA + off.r[s] + dAB + blk + qt * 2048), vf[s], dp);
                    }
                    // A rows = queries, B cols = keys -> acc[r] = S[q = 4g + r][key = li]
                    const int qv = qb * 32 + qt * 16 + 4 * g;
                    const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse2 + qv);
                    const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(Dq + qv);
                    const int js = jl - (r0 + qv);          // REL: the slot of (key, query r0 + qv), the rows behind it one slot lower each
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float p = REL ? __builtin_amdgcn_exp2f(__builtin_fmaf(sa[r], sl2, dbias[js - r]) - l4[r])
                                      : __builtin_amdgcn_exp2f(__builtin_fmaf(sa[r], SCALE_LOG2E, -l4[r]));
                        if (qedge && r0 + qv + r >= Tq) p = 0.f;
                        if (DROP) {
                            const float mk = drop_scale(headbase + (unsigned)(r0 + qv + r) * (unsigned)Tk + (unsigned)key, a.drop_seed, dth, dks);
                            pt[qt][r] = p * mk;
                            dst[qt][r] = p * (dp[r] * mk - d4[r]);
                        } else {
                            pt[qt][r] = p;
                            dst[qt][r] = p * (dp[r] - d4[r]);
                        }
                    }
                }
                const bf16x8_t pf = pack8(pt[0], pt[1]), dsf = pack8(dst[0], dst[1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    dv[dt] = mfma16(al_cols_frag(bufA + off.t[dt] + dAB + blk), pf, dv[dt]);
                    dk[dt] = mfma16(al_cols_frag(bufA + off.t[dt] + blk), dsf, dk[dt]);
                }
                if (REL && a.drel) {
#pragma unroll 1          // (unrolled, the two halves' sums are live together: 3 / 12 registers spilled at the 128 of two workgroups per CU)
                    for (int qt = 0; qt < 2; ++qt) {
                        const int qv = qb * 32 + qt * 16 + 4 * g, js = jl - (r0 + qv);
                        // d bias = dS summed along the diagonals, by all waves at once, in 64-bit fixed point: the DPP pre-sum of
                        // attn_bwd_kernel (lane j ends with d(3, j) + d(2, j - 1) + d(1, j - 2) + d(0, j - 3), the diagonal of
                        // (key_j, row 3); lanes 13 .. 15 hold a second value for the six elements that fall off the row's right edge)
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = (key < Tk && !(qedge && r0 + qv + r >= Tq)) ? dst[qt][r] : 0.f;
                        auto shr1 = [](float x) {
                            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x111, 0xf, 0xf, true));
                        };
                        float t = v[0];
                        t = v[1] + shr1(t);
                        t = v[2] + shr1(t);
                        t = v[3] + shr1(t);
                        if (t != 0.f) atomicAdd(&ddiag[js - 3], att_drel_fix(t));
                        const float w1 = li >= 14 ? v[1] : 0.f, w2 = li == 15 ? v[2] : 0.f;
                        float wv = li >= 13 ? v[0] : 0.f;
                        wv += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, w1), 0x101, 0xf, 0xf, true));   // row_shl:1
                        wv += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, w2), 0x102, 0xf, 0xf, true));   // row_shl:2
                        if (li >= 13 && wv != 0.f) atomicAdd(&ddiag[js], att_drel_fix(wv));
                    }
                }
            }
        }
        if (c + 1 < nch) put(lds + ((c + 1) & 1) * BUF, r0 + AL_QC);
        __syncthreads();
    }
    if (stores) {
        if (XL && key >= kvalid) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dv[dt] = zero4;
                dk[dt] = zero4;
            }
        }
        const bool live = key < Tk;
        const long krow = ((long)m * Tk + min(key, Tk - 1)) * a.dkv_ld + h * ATT_D;
        att_store_tile(dk, oscale, a.dk + krow, live, g);
        att_store_tile(dv, 1.0f, a.dv + krow, live, g);
    }
    if (REL && a.drel) {
        // diagonals -> buckets, still in fixed point (any order gives the same integer), then ONE conversion to fp32 per bucket.  With a
        // partial buffer the workgroup stores its nbuckets sums, zeros included, as the partial of (item, key block); the launcher adds
        // the partials into drel in that order (reduce_partials).  Without one: one float atomic per bucket, a counted lapse.
        __syncthreads();
        const int d0 = kblk * AL_ROWS - 36;
        for (int j = 36 + tid; j < nslot; j += AL_THREADS) {
            const unsigned long long v = ddiag[j];
            if (v && d0 + j < Tq + Tk - 1) atomicAdd(&bsum[a.rel_bucket[d0 + j]], v);
        }
        __syncthreads();
        for (int b = tid; b < a.nbuckets; b += AL_THREADS) {
            const float v = (float)(long long)bsum[b] * (1.0f / ATT_DREL_FIX);
            if (a.drel_part) a.drel_part[(((long)m * nkblk + kblk) * a.nbuckets + b) * H + h] = v;
            else if (v != 0.f) atomicAdd(a.drel + b * H + h, v);
        }
    }
}
__global__ __launch_bounds__(AL_THREADS, 4) void attn_long_dkdv_kernel(AttnArgs a, int nkblk) { al_dkdv_body<false, false>(a, nkblk); }
template <bool DROP>
__global__ __launch_bounds__(AL_THREADS, 4) void attn_xlong_dkdv_kernel(AttnArgs a, int nkblk) {
    al_dkdv_body<true, DROP>(a, nkblk);
}
template <bool DROP>
__global__ __launch_bounds__(AL_THREADS, 4) void attn_rlong_dkdv_kernel(AttnArgs a, int nkblk) {
    al_dkdv_body<false, DROP, true>(a, nkblk);
}

// ---------------- backward: dQ (phase 2 of attn_bwd_kernel, the keys streamed) ----------------
template <bool XL, bool DROP, bool REL = false>
DEVINL void al_dq_body(const AttnArgs& a, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int NL = AL_KV * 8 / AL_THREADS;
    constexpr int BUF = 2 * AL_KV * 128;
    const int H = a.H;
    const int qb = blockIdx.x % nqb, mh = blockIdx.x / nqb;
    const int m = mh / H, h = mh % H;
    long qr0;
    int Tq, Tk;          // Tk: the keys of the sweep (see al_fwd_body)
    al_item<XL>(a, m, qr0, Tq, Tk);
    if (XL && qb * AL_ROWS >= Tq) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned short* qbase = a.q + qr0 * a.q_ld + h * ATT_D;
    const unsigned short* kbase = a.k + (long)m * a.Tk * a.kv_ld + h * ATT_D;
    const unsigned short* vbase = a.v + (long)m * a.Tk * a.kv_ld + h * ATT_D;
    const unsigned short* obase = a.out + qr0 * a.out_ld + h * ATT_D;
    const unsigned short* dobase = a.dout + qr0 * a.out_ld + h * ATT_D;
    const float* lsebase = a.lse + ((long)m * H + h) * a.Tq;
    const unsigned dth = DROP ? drop_threshold(a.drop_p) : 0u;
    const float dks = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const int li = lane & 15, g = lane >> 4;
    const int qw0 = qb * AL_ROWS;                  // the workgroup's first query row (< Tq)
    const int q0 = qw0 + w * 16, q = q0 + li;
    const bool active = q0 < Tq;
    float* lse2 = reinterpret_cast<float*>(lds + 2 * BUF);      // [AL_ROWS] lse * log2 e, then [AL_ROWS] delta
    float* Dq = lse2 + AL_ROWS;
    const float sl2 = REL ? a.scale * LOG2EF : SCALE_LOG2E;
    const float oscale = REL ? a.scale : ATT_SCALE;
    const float* dbias = Dq + AL_ROWS + (Tq - 1 - min(q, Tq - 1));      // + key: the lane's row of the bias (see al_fwd_body)
    if (REL) al_fill_bias(Dq + AL_ROWS, a, h, 0, Tq + Tk - 1, Tq + Tk + 31, tid);
    u32x4_t rk[NL], rv[NL];
    al_load<AL_KV>(rk, kbase, a.kv_ld, 0, Tk, tid);
    al_load<AL_KV>(rv, vbase, a.kv_ld, 0, Tk, tid);
    {
        u32x4_t ro[AL_ROWS * 8 / AL_THREADS], rdo[AL_ROWS * 8 / AL_THREADS];
        al_load<AL_ROWS>(ro, obase, a.out_ld, qw0, Tq, tid);
        al_load<AL_ROWS>(rdo, dobase, a.out_ld, qw0, Tq, tid);
        if (tid < AL_ROWS) lse2[tid] = (qw0 + tid < Tq) ? lsebase[qw0 + tid] * LOG2EF : 0.f;
        al_delta<AL_ROWS>(Dq, ro, rdo, qw0, Tq, tid);
    }
    al_store<AL_KV>(lds, rk, 0, Tk, tid);
    al_store<AL_KV>(lds + AL_KV * 128, rv, 0, Tk, tid);
    bf16x8_t qf[2], dof[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        qf[s] = frag_rows_global(qbase, a.q_ld, q0, s, lane, Tq);
        dof[s] = frag_rows_global(dobase, a.out_ld, q0, s, lane, Tq);
    }
    __syncthreads();
    const float my_lse = lse2[w * 16 + li], my_D = Dq[w * 16 + li];
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = zero4;
    const AlOffs off = al_offs(li, g);
    const int nch = (Tk + AL_KV - 1) / AL_KV;
    for (int c = 0; c < nch; ++c) {
        const char* bufA = lds + (c & 1) * BUF;      // K; V sits AL_KV * 128 bytes behind it
        constexpr int dAB = AL_KV * 128;
        const int k0 = c * AL_KV;
        if (c + 1 < nch) {
            al_load<AL_KV>(rk, kbase, a.kv_ld, k0 + AL_KV, Tk, tid);
            al_load<AL_KV>(rv, vbase, a.kv_ld, k0 + AL_KV, Tk, tid);
        }
        if (active) {
            const int nkb = min(AL_KV / 32, (Tk - k0 + 31) >> 5);
            for (int kb = 0; kb < nkb; ++kb) {
                const int blk = kb * 4096;
                const bool edge = k0 + kb * 32 + 32 > Tk;
                f32x4_t dst[2];
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    f32x4_t sa = zero4, dp = zero4;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        sa = mfma16(al_rows_frag(bufA + off.r[s] + blk + kt * 2048), qf[s], sa);
                        dp = mfma16(al_rows_frag(bufA + off.r[s] + dAB + blk + kt * 2048), dof[s], dp);
                    }
                    // A rows = keys, B cols = queries -> acc[r] = S[key = 4g + r][q = li]
                    const float* bp = dbias + k0 + kb * 32 + kt * 16 + 4 * g;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        dst[kt][r] = REL ? __builtin_amdgcn_exp2f(__builtin_fmaf(sa[r], sl2, bp[r]) - my_lse)
                                         : __builtin_amdgcn_exp2f(__builtin_fmaf(sa[r], SCALE_LOG2E, -my_lse));
                    if (edge) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + kb * 32 + kt * 16 + 4 * g + r >= Tk) dst[kt][r] = 0.f;
                    }
                    if (DROP) {
                        const unsigned rowbase = (unsigned)((((long)m * H + h) * a.drop_tq + a.drop_q0 + q) * a.Tk);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dp[r] *= drop_scale(rowbase + (unsigned)(k0 + kb * 32 + kt * 16 + 4 * g + r), a.drop_seed, dth, dks);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[kt][r] = dst[kt][r] * (dp[r] - my_D);
                }
                const bf16x8_t dsf = pack8(dst[0], dst[1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) dq[dt] = mfma16(al_cols_frag(bufA + off.t[dt] + blk), dsf, dq[dt]);
            }
        }
        if (c + 1 < nch) {
            char* nx = lds + ((c + 1) & 1) * BUF;
            al_store<AL_KV>(nx, rk, k0 + AL_KV, Tk, tid);
            al_store<AL_KV>(nx + AL_KV * 128, rv, k0 + AL_KV, Tk, tid);
        }
        __syncthreads();
    }
    if (active)
        att_store_tile(dq, oscale, a.dq + (qr0 + min(q, Tq - 1)) * a.dq_ld + h * ATT_D, q < Tq, g);
}
__global__ __launch_bounds__(AL_THREADS, 4) void attn_long_dq_kernel(AttnArgs a, int nqb) { al_dq_body<false, false>(a, nqb); }
template <bool DROP>
__global__ __launch_bounds__(AL_THREADS, 4) void attn_xlong_dq_kernel(AttnArgs a, int nqb) {
    al_dq_body<true, DROP>(a, nqb);
}
template <bool DROP>
__global__ __launch_bounds__(AL_THREADS, 4) void attn_rlong_dq_kernel(AttnArgs a, int nqb) {
    al_dq_body<false, DROP, true>(a, nqb);
}

// ---------------- launchers: one forward, one backward for the three families ----------------
// (instantiated here so that the kernels stand in the code object family by family, as they always have)
template __global__ void attn_long_fwd_kernel<false>(AttnArgs, int);
template __global__ void attn_long_fwd_kernel<true>(AttnArgs, int);
template __global__ void attn_xlong_fwd_kernel<false>(AttnArgs, int);
template __global__ void attn_xlong_fwd_kernel<true>(AttnArgs, int);
template __global__ void attn_xlong_fwd_kernel<false, true>(AttnArgs, int);
template __global__ void attn_xlong_dkdv_kernel<false>(AttnArgs, int);
template __global__ void attn_xlong_dkdv_kernel<true>(AttnArgs, int);
template __global__ void attn_xlong_dq_kernel<false>(AttnArgs, int);
template __global__ void attn_xlong_dq_kernel<true>(AttnArgs, int);
enum AlFamily { AL_PLAIN, AL_XL, AL_REL };
static const int AL_FWD_LDS = 2 * 2 * AL_KV * 128;
static const int AL_DKDV_LDS = 2 * (2 * AL_QC * 128 + 2 * AL_QC * 4);
static const int AL_DQ_LDS = 2 * 2 * AL_KV * 128 + 2 * AL_ROWS * 4;
// LDS behind these buffers in the REL family: the bias table of the forward and dQ, the fixed-point sums and the bias slice of dK / dV
static int al_rel_tab_bytes(int seq) { return (2 * seq + 32) * 4; }
static int al_rel_dkdv_bytes(int seq) { return 64 * 8 + (seq + 164) * 12; }

// f16: AL_PLAIN (the fp16 forward of the towers), AL_XL without dropout (uniir_attn_general_fwd_f16 / uniir_onequery_fwd_f16) and
// AL_REL without dropout (uniir_attn_rel_fwd_long_f16)
static int al_launch_fwd(AlFamily fam, const AttnArgs& a, int batch, hipStream_t st, bool f16 = false) {
    const int nqb = (a.Tq + AL_ROWS - 1) / AL_ROWS;
    const long grid = (long)batch * a.H * nqb;
    if (grid > 0x7fffffffL) return UNIIR_ESHAPE;
    const dim3 g((unsigned)grid), b(AL_THREADS);
    const bool drop = a.drop_p > 0.f;
    if (fam == AL_PLAIN) {
        if (!f16) return att_launch<attn_long_fwd_kernel<false>>(AL_FWD_LDS, g, b, AL_FWD_LDS, st, a, nqb);
        return att_launch<attn_long_fwd_kernel<true>>(AL_FWD_LDS, g, b, AL_FWD_LDS, st, a, nqb);
    }
    if (fam == AL_XL) {
        if (f16) {
            if (drop) return UNIIR_EUNSUPPORTED;
            return att_launch<attn_xlong_fwd_kernel<false, true>>(AL_FWD_LDS, g, b, AL_FWD_LDS, st, a, nqb);
        }
        if (!drop) return att_launch<attn_xlong_fwd_kernel<false>>(AL_FWD_LDS, g, b, AL_FWD_LDS, st, a, nqb);
        return att_launch<attn_xlong_fwd_kernel<true>>(AL_FWD_LDS, g, b, AL_FWD_LDS, st, a, nqb);
    }
    const int sm = AL_FWD_LDS + al_rel_tab_bytes(a.Tq), mx = AL_FWD_LDS + al_rel_tab_bytes(ATT_LONG_SEQ_MAX);
    if (f16) {
        if (drop) return UNIIR_EUNSUPPORTED;
        return att_launch<attn_rlong_fwd_kernel<false, true>>(mx, g, b, sm, st, a, nqb);
    }
    if (!drop) return att_launch<attn_rlong_fwd_kernel<false>>(mx, g, b, sm, st, a, nqb);
    return att_launch<attn_rlong_fwd_kernel<true>>(mx, g, b, sm, st, a, nqb);
}

// dK / dV, then dQ
static int al_launch_bwd(AlFamily fam, const AttnArgs& a, int batch, hipStream_t st) {
    const int nkblk = (a.Tk + AL_ROWS - 1) / AL_ROWS, nqb = (a.Tq + AL_ROWS - 1) / AL_ROWS;
    const long nk = (long)batch * a.H * nkblk, nq = (long)batch * a.H * nqb;
    if (nk > 0x7fffffffL || nq > 0x7fffffffL) return UNIIR_ESHAPE;
    const dim3 gk((unsigned)nk), gq((unsigned)nq), b(AL_THREADS);
    const bool drop = a.drop_p > 0.f;
    int rc;
    if (fam == AL_PLAIN) {
        rc = att_launch<attn_long_dkdv_kernel>(AL_DKDV_LDS, gk, b, AL_DKDV_LDS, st, a, nkblk);
        if (rc) return rc;
        return att_launch<attn_long_dq_kernel>(AL_DQ_LDS, gq, b, AL_DQ_LDS, st, a, nqb);
    }
    if (fam == AL_XL) {
        if (!drop) rc = att_launch<attn_xlong_dkdv_kernel<false>>(AL_DKDV_LDS, gk, b, AL_DKDV_LDS, st, a, nkblk);
        else rc = att_launch<attn_xlong_dkdv_kernel<true>>(AL_DKDV_LDS, gk, b, AL_DKDV_LDS, st, a, nkblk);
        if (rc) return rc;
        if (!drop) return att_launch<attn_xlong_dq_kernel<false>>(AL_DQ_LDS, gq, b, AL_DQ_LDS, st, a, nqb);
        return att_launch<attn_xlong_dq_kernel<true>>(AL_DQ_LDS, gq, b, AL_DQ_LDS, st, a, nqb);
    }
    const int sk = AL_DKDV_LDS + al_rel_dkdv_bytes(a.Tq), mk = AL_DKDV_LDS + al_rel_dkdv_bytes(ATT_LONG_SEQ_MAX);
    const int sq = AL_DQ_LDS + al_rel_tab_bytes(a.Tq), mq = AL_DQ_LDS + al_rel_tab_bytes(ATT_LONG_SEQ_MAX);
    if (!drop) rc = att_launch<attn_rlong_dkdv_kernel<false>>(mk, gk, b, sk, st, a, nkblk);
    else rc = att_launch<attn_rlong_dkdv_kernel<true>>(mk, gk, b, sk, st, a, nkblk);
    if (rc) return rc;
    if (!drop) return att_launch<attn_rlong_dq_kernel<false>>(mq, gq, b, sq, st, a, nqb);
    return att_launch<attn_rlong_dq_kernel<true>>(mq, gq, b, sq, st, a, nqb);
}

// what the plain kernels take: dense rows, no mask, no bias, no dropout, the default scale
static bool attn_long_plain(const AttnArgs& a) {
    return !a.causal && !a.klen && !a.row_off && !a.kv_row_off && !a.rel_emb && a.drop_p == 0.f && a.scale == ATT_SCALE && a.Tq >= 1 &&
           a.Tk >= 1 && a.Tq <= ATT_LONG_SEQ_MAX && a.Tk <= ATT_LONG_SEQ_MAX;
}
int launch_attn_long_fwd(const AttnArgs& a, int batch, hipStream_t st, bool f16) {
    return attn_long_plain(a) ? al_launch_fwd(AL_PLAIN, a, batch, st, f16) : UNIIR_ESHAPE;
}
int launch_attn_long_bwd(const AttnArgs& a, int batch, hipStream_t st) {
    return attn_long_plain(a) ? al_launch_bwd(AL_PLAIN, a, batch, st) : UNIIR_ESHAPE;
}
// the general form's forward for another file (uniir_onequery_fwd, uniir_attn_general_fwd_f16 and uniir_onequery_fwd_f16 in
// attention.hip): what uniir_attention_fwd_long launches; the one-query callers alone may pass kv_row_off.  f16: no dropout
int launch_attn_xlong_fwd(const AttnArgs& a, int batch, hipStream_t st, bool f16) {
    if (a.causal || a.rel_emb || a.scale != ATT_SCALE || a.Tq < 1 || a.Tk < 1 || a.Tq > ATT_LONG_SEQ_MAX || a.Tk > ATT_LONG_SEQ_MAX ||
        (a.kv_row_off && (a.row_off || a.klen)))
        return UNIIR_ESHAPE;
    return al_launch_fwd(AL_XL, a, batch, st, f16);
}

// ---------------- the general form (uniir_attention_fwd_long / _bwd_long) ----------------
// Up to ATT_LONG_SEQ_MAX x ATT_LONG_SEQ_MAX: q_row_off == NULL is uniir_attention_fwd_ex / _bwd_ex with causal = 0, otherwise
// uniir_attention_fwd_rows / _bwd_rows with kv_packed = 0 (packed query rows, K / V dense [batch][tk]).  Every size runs the
// streaming kernels above; nothing is forwarded to the resident kernels.  Unlike those entry points, these test drop_p BEFORE
// batch == 0, refuse a NaN drop_p, and the backward tests the alignment of all eight pointers.
extern "C" int uniir_attention_fwd_long(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out,
                                        int64_t out_ld, float* lse, const int32_t* q_row_off, const int32_t* key_len, int32_t batch,
                                        int32_t tq, int32_t tk, int32_t heads, float drop_p, uint32_t drop_seed, void* stream) {
    if (att_null(q, k, v, out, lse) || batch < 0 || heads <= 0) return UNIIR_EINVAL;
    if (att_bad_drop_nan(drop_p)) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (tq < 1 || tk < 1 || tq > ATT_LONG_SEQ_MAX || tk > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_ld_not8(q_ld, kv_ld, out_ld)) return UNIIR_EALIGN;
    if (att_misaligned16(q, k, v, out)) return UNIIR_EALIGN;
    AttnArgs a = att_args_qkv(q, q_ld, k, v, kv_ld, out, out_ld, lse, tq, tk, heads, key_len);
    att_args_q_rows(a, q_row_off, 1);
    att_args_drop(a, drop_p, drop_seed);
    return al_launch_fwd(AL_XL, a, batch, (hipStream_t)stream);
}
extern "C" int uniir_attention_bwd_long(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, const void* out,
                                        const void* dout, int64_t out_ld, const float* lse, const int32_t* q_row_off,
                                        const int32_t* key_len, void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld,
                                        int32_t batch, int32_t tq, int32_t tk, int32_t heads, float drop_p, uint32_t drop_seed,
                                        void* stream) {
    if (att_null(q, k, v, out, dout, lse, dq, dk, dv) || batch < 0 || heads <= 0) return UNIIR_EINVAL;
    if (att_bad_drop_nan(drop_p)) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (tq < 1 || tk < 1 || tq > ATT_LONG_SEQ_MAX || tk > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_ld_not8(q_ld, kv_ld, out_ld, dq_ld, dkv_ld)) return UNIIR_EALIGN;
    if (att_misaligned16(q, k, v, out, dout, dq, dk, dv)) return UNIIR_EALIGN;
    AttnArgs a = att_args_qkv(q, q_ld, k, v, kv_ld, out, out_ld, lse, tq, tk, heads, key_len);
    att_args_q_rows(a, q_row_off, 1);
    att_args_qkv_bwd(a, dout, dq, dq_ld, dk, dv, dkv_ld);
    att_args_drop(a, drop_p, drop_seed);
    return al_launch_bwd(AL_XL, a, batch, (hipStream_t)stream);
}

// ---------------- T5-style self-attention (uniir_attention_rel_fwd_long / _rel_bwd_long) ----------------
// uniir_attention_rel_fwd / _rel_bwd for 1 <= seq <= ATT_LONG_SEQ_MAX: every size runs the streaming kernels above, nothing is
// forwarded to the resident kernels.  drop_p before batch == 0 and NaN as above; and these test alignment, which rel_fwd / rel_bwd do not.
extern "C" int uniir_attention_rel_fwd_long(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                                            int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, float drop_p,
                                            uint32_t drop_seed, void* stream) {
    if (att_null(qkv, out, lse, rel_emb, rel_bucket) || batch < 0 || heads <= 0 || nbuckets <= 0 || nbuckets > 64) return UNIIR_EINVAL;
    if (att_bad_drop_nan(drop_p)) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (seq < 1 || seq > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_misaligned16(qkv, out)) return UNIIR_EALIGN;
    AttnArgs a = att_args_packed(qkv, out, lse, seq, heads, 0, scale);
    att_args_rel(a, rel_emb, rel_bucket, nbuckets);
    att_args_drop(a, drop_p, drop_seed);
    return al_launch_fwd(AL_REL, a, batch, (hipStream_t)stream);
}
// ... on fp16 tensors, forward only and without dropout: attn_rlong_fwd_kernel<false, true> at every size.  The checks of the call
// above minus its dropout ones.  (P <= 2^8 in fp16: see attn_fwd_kernel -- the same deferred maximum on the same folded logits.)
extern "C" int uniir_attn_rel_fwd_long_f16(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                                           int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, void* stream) {
    if (att_null(qkv, out, lse, rel_emb, rel_bucket) || batch < 0 || heads <= 0 || nbuckets <= 0 || nbuckets > 64) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (seq < 1 || seq > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_misaligned16(qkv, out)) return UNIIR_EALIGN;
    AttnArgs a = att_args_packed(qkv, out, lse, seq, heads, 0, scale);
    att_args_rel(a, rel_emb, rel_bucket, nbuckets);
    return al_launch_fwd(AL_REL, a, batch, (hipStream_t)stream, true);
}
static int al_launch_rel_bwd(const AttnArgs& a, int batch, hipStream_t st) { return al_launch_bwd(AL_REL, a, batch, st); }
extern "C" int uniir_attention_rel_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                            const float* rel_emb, const int32_t* rel_bucket, int32_t nbuckets, float scale,
                                            float* drel, int32_t batch, int32_t seq, int32_t heads, float drop_p, uint32_t drop_seed,
                                            void* stream) {
    if (att_null(qkv, out, dout, lse, dqkv, rel_emb, rel_bucket) || batch < 0 || heads <= 0 || nbuckets <= 0 || nbuckets > 64)
        return UNIIR_EINVAL;
    if (att_bad_drop_nan(drop_p)) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (seq < 1 || seq > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_misaligned16(qkv, out, dout, dqkv)) return UNIIR_EALIGN;
    const int nkblk = (seq + AL_ROWS - 1) / AL_ROWS;
    if ((long)batch * heads * nkblk > 0x7fffffffL) return UNIIR_ESHAPE;          // before the scratch is asked for: a refused call counts nothing
    AttnArgs a = att_args_packed(qkv, out, lse, seq, heads, 0, scale);
    att_args_packed_bwd(a, dout, dqkv);
    att_args_rel(a, rel_emb, rel_bucket, nbuckets);
    att_args_drop(a, drop_p, drop_seed);
    // one partial per (item, key block): [item][key block][bucket][head]
    return attention_rel_bwd_tail(a, drel, (long)batch * nkblk, batch, (hipStream_t)stream, al_launch_rel_bwd);
}
