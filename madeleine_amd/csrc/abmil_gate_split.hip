// abmil_gate_split.hip -- A2 (gated attention scores, reference madeleine/models/abmil.py:41-68 called per head from
// madeleine/models/Model.py:406-409) forward and backward with the three contractions on the split-fp16 engine (split_engine.hpp):
// fp32 values, fp32-level accuracy, 3 v_mfma_f32_32x32x16_f16 per 16 k instead of 8 v_mfma_f32_32x32x2_f32.  Same maths, same
// dropout counter hash, same partial-score / finalize / slab-reduction scheme as abmil_gate.hip (whose kernels remain the 'fp32'
// GEMM mode); the epilogues are fp32.
//   forward : A = image(E) rows of head c (K = 512)      B = image([Wa;Wb]) rows (a j | b j)     fused tanh / sigmoid / dropout / wc
//   dz      : d(za)|d(zb) written as an IMAGE directly by the HBM-bound pass (scale from the rigorous bound max|ds| max|wc| / (1-p)^2)
//   dX      : A = image(dz) rows (t, c) (K = 1024)       B = image([Wa;Wb]^T) rows e              dE (+)= . + pooling term
//   dW      : TN over tokens: A = image(E) head columns, B = image(dz) head columns              slabs -> gate_reduce_w
#include "split_engine.hpp"
#include "gate_host.hpp"

namespace mdl {

// ---- weight images --------------------------------------------------------------------------------------------------------------------
// sc[1] = max(|Wa|, |Wb|) (sp_absmax on both), sc[0] = its scale.
// WK [H][1024 rows: a j 0..511 | b j 0..511][512 k]: the forward's B operand
__global__ __launch_bounds__(256) void sp_gate_wk_kernel(const float* __restrict__ Wa, const float* __restrict__ Wb, char* __restrict__ WK,
                                                         int H, const float* __restrict__ sc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over H * 1024 * 64 groups of 8 k
    if (i >= (int64_t)H * 1024 * 64) return;
    const int k = (int)(i % 64) * 8, r = (int)((i / 64) % 1024), c = (int)(i / (64 * 1024));
    const float* src = (r < HID) ? Wa + ((int64_t)c * HID + r) * HID + k : Wb + ((int64_t)c * HID + r - HID) * HID + k;
    const float s = sc[0];
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
    const float v[8] = {x0.x * s, x0.y * s, x0.z * s, x0.w * s, x1.x * s, x1.y * s, x1.z * s, x1.w * s};
    u32x4 hi, lo;
    sp_split8(v, hi, lo);
    char* row = WK + ((int64_t)c * 1024 + r) * (HID * 4);
    *reinterpret_cast<u32x4*>(row + sp_img_off(k, 0)) = hi;
    *reinterpret_cast<u32x4*>(row + sp_img_off(k, 1)) = lo;
}
// WN [H][512 rows e][1024 columns: a j | b j] = [Wa;Wb]^T: the dX product's B operand   (32 x 32 LDS transpose)
__global__ __launch_bounds__(256) void sp_gate_wn_kernel(const float* __restrict__ Wa, const float* __restrict__ Wb, char* __restrict__ WN,
                                                         const float* __restrict__ sc) {
    __shared__ float tile[32][33];
    const int c = blockIdx.z, jb = blockIdx.y * 32, eb = blockIdx.x * 32;  // jb over 1024 (a | b), eb over 512
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* __restrict__ W = (jb < HID) ? Wa + ((int64_t)c * HID + jb) * HID : Wb + ((int64_t)c * HID + jb - HID) * HID;
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[ty + i * 8][tx] = W[(int64_t)(ty + i * 8) * HID + eb + tx];   // tile[j][e]
    __syncthreads();
    if (threadIdx.x < 128) {
        const int e = threadIdx.x >> 2, g = threadIdx.x & 3;   // row e, 8 consecutive j
        const float s = sc[0];
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = tile[g * 8 + u][e] * s;
        u32x4 hi, lo;
        sp_split8(v, hi, lo);
        char* row = WN + ((int64_t)c * HID + eb + e) * (1024 * 4);
        *reinterpret_cast<u32x4*>(row + sp_img_off(jb + g * 8, 0)) = hi;
        *reinterpret_cast<u32x4*>(row + sp_img_off(jb + g * 8, 1)) = lo;
    }
}
// out[0] = scale for a bound in[0] * in[1] * mult (dz: max|ds| * max|wc| / (1-p)^2); out[1] = the bound
__global__ void sp_bound_scale_kernel(const float* __restrict__ in, float mult, float* __restrict__ out) {
    const float b = in[0] * in[1] * mult;
    out[1] = b;
    out[0] = sp_scale_for(b);
}

// ================================================================================================
// forward
// ================================================================================================
// Tile: 256 tokens x (128 a | 128 b) gate columns j0 .. j0 + 127 of head c.  Tile column n = wn * SP_WCOLS + ct * 32 + l with the first
// SPNCT / 2 column tiles of a wave = a columns j0 + wn * (16 SPNCT) + ct * 32 + l and the second half = the b columns of the same j, so that
// a wave holds za and zb of the same (token, j) in acc[rt][cp] / acc[rt][SPNCT / 2 + cp].
// Round 5: persistent workgroups.  With one workgroup per CU (128 KiB of stages) nothing overlaps a tile's prologue -- workgroup launch,
// the first block's memory latency -- with the previous tile.  A persistent workgroup runs PER tiles back to back and requests the NEXT
// tile's first block into stage 0 before the epilogue of the current one; the epilogue stages through stage 1 (sp_stage1_tile) and the
// row sums have their own LDS.  Same arithmetic in the same order: bit-identical to one workgroup per tile.
//   PMODE 0: one tile per workgroup (round 4)
//   PMODE 1: the GATE_JT column tiles of one (token tile, head): the E tile is re-read by the same CU GATE_JT times in a row
//   PMODE 2: GATE_PT consecutive token tiles of one (column tile, head): the weight tile stays, and the GATE_JT workgroups of the same
//            token tiles still run side by side on one XCD (they share each E tile through its L2, as in PMODE 0)
// (default MDL_GATE_SP_PMODE, switches.hpp)
constexpr int GATE_PT = 4;
// NA = 3 (round 6; one tile per workgroup only): sp_nt_mainloop3 on SmemSP3 -- the LDS-DMA pieces spread over the chunk; the epilogue's
// transposes then use A[0] / A[1] and the row sums B[0] of the drained ring (160 KiB leave no room for a separate array).
template <int DM, bool SAVE, int PMODE, int NA = 2>
__global__ __launch_bounds__(SP_THREADS) void sp_gate_fwd_kernel(const char* __restrict__ Ei, int64_t e_rsb, const float* __restrict__ e_sc,
                                                          const char* __restrict__ WK, const float* __restrict__ w_sc,
                                                          const float* __restrict__ ba, const float* __restrict__ bb,
                                                          const float* __restrict__ wc, float* __restrict__ part,
                                                          float* __restrict__ act_a, float* __restrict__ act_b, int64_t T, int H,
                                                          int n_ttiles, DropCfg drop) {
    static_assert(NA == 2 || PMODE == 0, "the three-stage ring serves one tile per workgroup");
    __shared__ SmemSPn<NA> sm;
    __shared__ float sred_own[NA == 2 ? SP_WN * SPM : 1];   // [SP_WN][256 rows]
    float* sred_s = NA == 2 ? sred_own : reinterpret_cast<float*>(&sm.B[0][0]);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / SP_WN, wn = wave % SP_WN;
    const XcdHead xh = xcd_head(blockIdx.x, H);
    const int c = xh.c;
    // the workgroup's tiles: (token tile tt_of(k), column tile jt_of(k)), k = 0 .. n_k - 1
    constexpr int n_k = PMODE == 1 ? GATE_JT : PMODE == 2 ? GATE_PT : 1;
    auto tt_of = [&](int k) { return (PMODE == 1 ? xh.li : PMODE == 2 ? (xh.li / GATE_JT) * GATE_PT + k : xh.li / GATE_JT) * xh.nshare + xh.share; };
    auto jt_of = [&](int k) { return PMODE == 1 ? k : xh.li % GATE_JT; };
    if (tt_of(0) >= n_ttiles) return;  // block-uniform

    constexpr int HALF = SPNCT / 2;   // a (= b) column tiles per wave
    uint32_t voB[SP_PW];
#pragma unroll
    for (int i = 0; i < SP_PW; ++i) {
        int row, ch;
        sp_nt_slot(wave, i, lane, row, ch);
        // tile row (= tile column of the product) -> row of the head's [a | b] weight block, relative to the tile's first gate column j0
        const int wv = row / SP_WCOLS, ct = (row >> 5) % SPNCT;
        const int wrow = (ct / HALF) * HID + wv * (32 * HALF) + (ct % HALF) * 32 + (row & 31);
        voB[i] = (uint32_t)(wrow * (HID * 4) + ch * 16);
    }
    auto a_offsets = [&](int64_t t0, uint32_t (&vo)[SP_PW]) {   // rows past T re-read the last valid row (discarded)
#pragma unroll
        for (int i = 0; i < SP_PW; ++i) {
            int row, ch;
            sp_nt_slot(wave, i, lane, row, ch);
            int64_t ra = row;
            if (t0 + ra > T - 1) ra = T - 1 - t0;
            vo[i] = (uint32_t)(ra * e_rsb + ch * 16);
        }
    };
    const float inv = 1.f / (e_sc[0] * w_sc[0]);
    const int l32 = lane & 31;
    float* tile = NA == 2 ? sp_stage1_tile(sm, wave) : reinterpret_cast<float*>(&sm.A[wave / (SP_WAVES / 2)][(wave % (SP_WAVES / 2)) * 8192]);
    float* sred = sred_s + wn * SPM + wm * 128;
    const int g8 = lane & 7, r8 = lane >> 3;

    for (int k = 0; k < n_k; ++k) {
    const int tt = tt_of(k), jt = jt_of(k);
    if (tt >= n_ttiles) break;   // block-uniform (PMODE 2: a short last group)
    const int64_t t0 = (int64_t)tt * SPM;
    const int j0 = jt * 128;
    const char* baseA = Ei + t0 * e_rsb + (int64_t)c * (HID * 4);
    const char* baseB = WK + ((int64_t)c * 1024 + j0) * (HID * 4);
    uint32_t voA[SP_PW];
    a_offsets(t0, voA);
    SpAcc acc;
    sp_zero(acc);
    auto dma = [&](int st, int f, int piece) {
        const int i = piece % SP_PW;
        if (piece < SP_PW) glds16_s(voA[i], sp_uniform(baseA + (int64_t)f * 128), lds_addr_of(&sm.A[st][(wave * SP_PW + i) * 1024]));
        else glds16_s(voB[i], sp_uniform(baseB + (int64_t)f * 128), lds_addr_of(&sm.B[st][(wave * SP_PW + i) * 1024]));
    };
    if constexpr (NA == 3) sp_nt_mainloop3(sm, acc, HID / 32, wm, wn, lane, dma);
    else sp_nt_mainloop(sm, acc, HID / 32, wm, wn, lane, dma, k > 0);
    if (k + 1 < n_k && tt_of(k + 1) < n_ttiles) {   // the next tile's first block travels during this epilogue
        const int64_t t0n = (int64_t)tt_of(k + 1) * SPM;
        const char* baseAn = Ei + t0n * e_rsb + (int64_t)c * (HID * 4);
        const char* baseBn = WK + ((int64_t)c * 1024 + jt_of(k + 1) * 128) * (HID * 4);
        uint32_t voAn[SP_PW];
        a_offsets(t0n, voAn);
#pragma unroll
        for (int piece = 0; piece < SP_NP; ++piece) {
            const int i = piece % SP_PW;
            if (piece < SP_PW) glds16_s(voAn[i], sp_uniform(baseAn), lds_addr_of(&sm.A[0][(wave * SP_PW + i) * 1024]));
            else glds16_s(voB[i], sp_uniform(baseBn), lds_addr_of(&sm.B[0][(wave * SP_PW + i) * 1024]));
        }
    }

    // ---- epilogue: 4 x HALF passes (rt, cp) of a 32-row x (32 a | 32 b)-column block through the wave's LDS tile (as abmil_gate.hip)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int cp = 0; cp < HALF; ++cp) {
            const int jc = j0 + wn * (32 * HALF) + cp * 32;   // first gate column of this pass
            // pre-activation = acc * inv + bias, folded into the exponent's FMA (gate_tanh_pre / gate_sigmoid_pre, common.hpp)
            const float ta = 2.f * MDL_LOG2E * ba[c * HID + jc + l32], tb = -MDL_LOG2E * bb[c * HID + jc + l32];
            const float sa2 = 2.f * MDL_LOG2E * inv, sb1 = -MDL_LOG2E * inv;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tile[acc_row(r, lane) * 64 + l32] = gate_tanh_pre(acc[rt][cp][r], sa2, ta);
                tile[acc_row(r, lane) * 64 + 32 + l32] = gate_sigmoid_pre(acc[rt][HALF + cp][r], sb1, tb);
                if ((r & 3) == 3) SP_SB();
            }
            // score term of an element: keep_a keep_b / (1-p)^2 a b wc -- the two dropout factors folded into wc, ONE select per pair
            const f32x4 wc4 = *reinterpret_cast<const f32x4*>(wc + c * HID + jc + g8 * 4) * (drop.inv * drop.inv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = i * 8 + r8;
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&tile[row * 64 + g8 * 4]);
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(&tile[row * 64 + 32 + g8 * 4]);
                float sum = 0.f;
                if (t0 + wm * 128 + rt * 32 + row < T) {
                    const int64_t idx = ((t0 + wm * 128 + rt * 32) * H + c) * HID + jc + (uint32_t)(row * H * HID + g8 * 4);
                    const uint32_t rkey = drop_row_key(drop, idx);   // idx % 4 == 0: the 4 elements share the high word
                    if (SAVE) {
                        *reinterpret_cast<f32x4*>(act_a + idx) = a4;
                        *reinterpret_cast<f32x4*>(act_b + idx) = b4;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bool keep_a, keep_b;
                        gate_keep2_fwd<DM>(drop, idx, e, rkey, keep_a, keep_b);
                        const float ab = a4[e] * b4[e];
                        sum = fmaf((keep_a && keep_b) ? ab : 0.f, wc4[e], sum);
                    }
                }
                sum += __shfl_xor(sum, 1, 64);
                sum += __shfl_xor(sum, 2, 64);
                sum += __shfl_xor(sum, 4, 64);
                if (g8 == 0) {
                    if (cp == 0) sred[rt * 32 + row] = sum;
                    else sred[rt * 32 + row] += sum;
                }
                SP_SB();
            }
        }
    __syncthreads();
    for (int rr = tid; rr < SPM; rr += SP_THREADS) {
        const int64_t t = t0 + rr;
        float v = sred_s[rr];
#pragma unroll
        for (int w = 1; w < SP_WN; ++w) v += sred_s[w * SPM + rr];
        if (t < T) part[(t * H + c) * GATE_JT + jt] = v;
    }
    }   // k (the next tile's main loop has barriers between these reads of sred_s and its epilogue's writes)
}

// ================================================================================================
// backward, stage 1: d(za) | d(zb) as a split image [T + 32][H][1024] (+ the column sums), scale dz_sc[0] from the bound
// ================================================================================================
// Workgroup = DZ_ROWS token rows x ALL heads (64 H threads: thread = (head, 8 columns)): every row is one contiguous 2 KB H read of
// each activation and one contiguous 4 KB H write of the image (a workgroup per head touched 2 KB of every 8 KB).
template <int DM>   // dropout mode, as the forward kernels (gate_keep2_fwd)
__global__ __launch_bounds__(64 * MDL_MAX_HEADS) void sp_gate_dz_kernel(const float* __restrict__ wc, const float* __restrict__ act_a,
                                                         const float* __restrict__ act_b, const float* __restrict__ d_scores,
                                                         char* __restrict__ dzi, const float* __restrict__ dz_sc,
                                                         float* __restrict__ slabV, int64_t T, int H, DropCfg drop, int rows_per_wg) {
    // Round 5: lane q of head c owns columns 4q .. 4q + 3 and 256 + 4q .. 256 + 4q + 3 of its head (fully coalesced float4 loads: one
    // instruction of the wave = 1 KiB), and the image goes out through sp_img_store4's pair exchange (whole 128-B lines per store
    // instruction).  Round 4 had 8 consecutive columns per lane: 32-B loads and 16 B + 16 B stores, the half-line pattern that streams
    // 4.8 TB/s where this order streams 5.2-5.4 (tools/micro/hbm_rate.hip patterns).  Same values, same summation order per column.
    constexpr int NH = 2, VEC = 4;   // column halves per lane x columns per float4
    const int tid = threadIdx.x, q = tid & 63, c = tid >> 6;
    const int64_t bx = blockIdx.x;
    const int64_t r0 = bx * rows_per_wg;
    int64_t r1 = r0 + rows_per_wg;
    if (r1 > T) r1 = T;
    const float s = dz_sc[0];
    f32x4 vw[NH], sa[NH], sb[NH], sw[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        vw[h] = *reinterpret_cast<const f32x4*>(wc + c * HID + h * 256 + q * VEC);
        sa[h] = sb[h] = sw[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float sds = 0.f;
    constexpr int UNR = 2;   // 2 rows x (a, b) x 2 x 16 B = 8 loads in flight per thread
    for (int64_t rb = r0; rb < r1; rb += UNR) {
        f32x4 va[UNR][NH], vb[UNR][NH];
        float ds[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t r = rb + u;
            const bool ok = r < r1;
            const int64_t o = ((ok ? r : rb) * H + c) * HID + q * VEC;
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                va[u][h] = ld4_nt(act_a + o + h * 256);
                vb[u][h] = ld4_nt(act_b + o + h * 256);
            }
            ds[u] = ok ? d_scores[r * H + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t r = rb + u;
            if (r < r1) {   // block-uniform
                const int64_t o = (r * H + c) * HID + q * VEC;
                const uint32_t rkey = drop_row_key(drop, o);   // the head's 512 elements share the high word
                char* row = dzi + (r * H + c) * (int64_t)(1024 * 4);
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    f32x4 za, zb;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        float w, a, b;
                        gate_dz_t<DM>(drop, ds[u], vw[h][i], va[u][h][i], vb[u][h][i], o + h * 256, i, rkey, a, b, w);
                        sw[h][i] += w;
                        sa[h][i] += a;
                        sb[h][i] += b;
                        za[i] = a;
                        zb[i] = b;
                    }
                    sp_img_store4(row, h * 256 + q * VEC, za, s);
                    sp_img_store4(row, HID + h * 256 + q * VEC, zb, s);
                }
                sds += ds[u];
            }
        }
    }
    float* __restrict__ o = slabV + (bx * H + c) * 4 * HID + q * VEC;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        *reinterpret_cast<f32x4*>(o + h * 256) = sa[h];
        *reinterpret_cast<f32x4*>(o + HID + h * 256) = sb[h];
        *reinterpret_cast<f32x4*>(o + 2 * HID + h * 256) = sw[h];
    }
    if (q == 0) o[3 * HID] = sds;
}

// ================================================================================================
// backward, stage 2: dE[t, c, n0 + n] (+)= sum_j dz[t, c, j] WN[c][n0 + n][j]  (+ pooling term), K = 1024
// ================================================================================================
template <int TERMS, int NA = 2>   // NA = 3: sp_nt_mainloop3 on SmemSP3 (the epilogue works in the first 128 KiB of the drained ring)
__global__ __launch_bounds__(SP_THREADS) void sp_gate_dx_kernel(const char* __restrict__ dzi, const float* __restrict__ dz_sc,
                                                         const char* __restrict__ WN, const float* __restrict__ w_sc,
                                                         float* __restrict__ dE, int64_t ldE, int accumulate, int64_t T, int H,
                                                         PoolTerm pt, float* __restrict__ absmax_out) {
    __shared__ SmemSPn<NA> sm3;
    SmemSP& sm = reinterpret_cast<SmemSP&>(sm3);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / SP_WN, wn = wave % SP_WN;
    const XcdHead xh = xcd_head(blockIdx.x, H);
    const int nt = xh.li % 2, c = xh.c, tt = (xh.li / 2) * xh.nshare + xh.share;
    const int64_t t0 = (int64_t)tt * SPM;
    if (t0 >= T) return;  // block-uniform
    const int n0 = nt * SPN;

    const uint32_t rowA = (uint32_t)H * 4096u;
    const char* baseA = dzi + (t0 * H + c) * (int64_t)4096;
    const char* baseB = WN + ((int64_t)c * HID + n0) * 4096;
    uint32_t voA[SP_PW], voB[SP_PW];
#pragma unroll
    for (int i = 0; i < SP_PW; ++i) {
        int row, ch;
        sp_nt_slot(wave, i, lane, row, ch);
        int64_t ra = row;
        if (t0 + ra > T - 1) ra = T - 1 - t0;
        voA[i] = (uint32_t)ra * rowA + ch * 16;
        voB[i] = (uint32_t)row * 4096u + ch * 16;
    }
    // fused A3 term: the softmax weight and the d_pooled row of every tile row, ONCE per row (thread r < 256 owns row r; the loads
    // fly behind the main loop) -- per output vector this was a 64-bit division, three dependent loads and an exp: 8,400 epilogue
    // instructions per wave against the main loop's 5,000
    float row_w = 0.f;
    int row_off = 0;
    if (pt.scores && tid < SPM && t0 + tid < T) {
        int bag;
        row_w = pool_term_weight(pt, t0 + tid, c, H, bag);
        row_off = (bag * H + c) * HID;
    }
    SpAcc acc;
    sp_zero(acc);
    auto dma = [&](int st, int f, int piece) {
        const int i = piece % SP_PW;
        if (piece < SP_PW) glds16_s(voA[i], sp_uniform(baseA + (int64_t)f * 128), lds_addr_of(&sm3.A[st][(wave * SP_PW + i) * 1024]));
        else glds16_s(voB[i], sp_uniform(baseB + (int64_t)f * 128), lds_addr_of(&sm3.B[st][(wave * SP_PW + i) * 1024]));
    };
    if constexpr (NA == 3) sp_nt_mainloop3<TERMS>(sm3, acc, 1024 / 32, wm, wn, lane, dma);
    else sp_nt_mainloop<TERMS>(sm3, acc, 1024 / 32, wm, wn, lane, dma);
    const float inv = 1.f / (dz_sc[0] * w_sc[0]);
    float amax = 0.f;
    char* ob = reinterpret_cast<char*>(dE + t0 * ldE + (int64_t)c * HID + n0);
    const uint32_t ld4 = (uint32_t)ldE * 4u;
    // row factors -> LDS behind the epilogue's transpose area (the first 64 KiB of the staging memory, free after the main loop)
    float* rw_s = reinterpret_cast<float*>(&sm.B[0][0]);
    int* ro_s = reinterpret_cast<int*>(&sm.B[0][SPM * 4]);
    if (pt.scores) {
        if (tid < SPM) {
            rw_s[tid] = row_w;
            ro_s[tid] = row_off;
        }
        __syncthreads();
    }
    const float* dpb = pt.d_pooled + n0;
    // One epilogue per mode (sp_epilogue_rows_ld, split_engine.hpp): no pooling term | the tile inside ONE bag (bags are contiguous: its
    // first and last valid rows share a bag), the lane's d_pooled vector loaded once | rows of several bags, the d_pooled vectors of a
    // group of rows loaded ahead of the group; the old dE likewise.  No memory wait between the stores of a group.
    const int rows_valid = t0 + SPM <= T ? SPM : (int)(T - t0);
    constexpr int DX_ACC = 1, DX_POOL = 2, DX_ONE_BAG = 4;
    int mode = accumulate ? DX_ACC : 0;
    if (pt.scores) mode |= __builtin_amdgcn_readfirstlane(ro_s[0] == ro_s[rows_valid - 1]) ? DX_POOL | DX_ONE_BAG : DX_POOL;
    static_assert(SPNCT == 2, "one column vector per lane");
    const int lcol = wn * SP_WCOLS + (lane & 15) * 4;
    sp_mode_switch<3>(mode, [&](auto tag) {
        constexpr int MD = decltype(tag)::value;
        if constexpr (!(MD & DX_ONE_BAG) || (MD & DX_POOL)) {   // (one bag without a pooling term: no such mode)
            f32x4 dp1 = {};
            if constexpr (MD & DX_ONE_BAG) dp1 = *reinterpret_cast<const f32x4*>(dpb + (ro_s[0] + lcol));
            f32x4 dpv[2], oc[2];
            auto pre = [&](int j, int row, int col, int, bool valid) {   // (an invalid row reads row 0 instead; its value is dropped)
                const int rl = valid ? row : 0;
                if constexpr ((MD & DX_POOL) && !(MD & DX_ONE_BAG)) dpv[j] = *reinterpret_cast<const f32x4*>(dpb + (ro_s[rl] + col));
                if constexpr (MD & DX_ACC) oc[j] = *reinterpret_cast<const f32x4*>(ob + (int64_t)rl * ld4 + (uint32_t)col * 4u);
            };
            auto emit = [&](int j, int row, int col, int, const f32x4& v, bool valid) {
#pragma clang fp contract(off)
                f32x4 r = v * inv;
                if constexpr (MD & DX_POOL) {  // + w[t,c] * d_pooled[bag(t), c, :]  (cache-resident row)
                    const float w = rw_s[row];
                    const f32x4 dp = (MD & DX_ONE_BAG) ? dp1 : dpv[j];
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = fmaf(w, dp[i], r[i]);
                }
                if constexpr (MD & DX_ACC) r += oc[j];
                sp_keep(r);
                if (valid) {
                    *reinterpret_cast<f32x4*>(ob + (int64_t)row * ld4 + (uint32_t)col * 4u) = r;
                    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(r.x), fabsf(r.y))), fmaxf(fabsf(r.z), fabsf(r.w)));
                }
            };
            if (rows_valid == SPM) sp_epilogue_rows_ld<true, 2>(acc, sm, wave, wm, wn, lane, SPM, pre, emit);
            else sp_epilogue_rows_ld<false, 2>(acc, sm, wave, wm, wn, lane, rows_valid, pre, emit);
        }
    });
    if (absmax_out) sp_block_absmax(absmax_out, amax, reinterpret_cast<float*>(&sm.B[1][0]));   // B[0] holds the row factors
}

// ================================================================================================
// backward, stage 3: slabW[sp][c][k' 512][1024: a | b] = sum_{t in split} E[t, c, k'] dz[t, c, n]      (TN over tokens)
// ================================================================================================
template <int TERMS, int NA = 2>   // NA = 3: sp_tn_mainloop3 on SmemSP3
__global__ __launch_bounds__(SP_THREADS) void sp_gate_dw_kernel(const char* __restrict__ Ei, int64_t e_rsb, const float* __restrict__ e_sc,
                                                         const char* __restrict__ dzi, const float* __restrict__ dz_sc,
                                                         float* __restrict__ slabW, int64_t T, int H, int64_t tok_per_split,
                                                         int n_splits) {
    __shared__ SmemSPn<NA> sm3;
    SmemSP& sm = reinterpret_cast<SmemSP&>(sm3);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / SP_WN, wn = wave % SP_WN;
    const XcdHead xh = xcd_head(blockIdx.x, H);
    const int kt = xh.li % 2, ntile = (xh.li / 2) % 4, c = xh.c, sp = (xh.li / 8) * xh.nshare + xh.share;
    if (sp >= n_splits) return;  // block-uniform
    const int i0 = kt * SPM, n0 = ntile * SPN;
    const int64_t ts = (int64_t)sp * tok_per_split;
    int64_t te = ts + tok_per_split;
    if (te > T) te = T;
    const int64_t nch = (te > ts) ? (te - ts + SPK - 1) / SPK : 0;

    uint32_t tokq[SP_PW], coA[SP_PW], coB[SP_PW];
#pragma unroll
    for (int q = 0; q < SP_PW; ++q) {
        const int kr = (wave * SP_PW + q) * 2 + (lane >> 5), p = kr >> 5, src = (lane & 31) ^ ((kr & 3) << 2);
        tokq[q] = kr & 31;
        coA[q] = (uint32_t)sp_img_off(i0 + src * 8, p);
        coB[q] = (uint32_t)sp_img_off(n0 + src * 8, p);
    }
    const uint32_t rowB = (uint32_t)H * 4096u;
    const char* baseA = Ei + ts * e_rsb + (int64_t)c * (HID * 4);
    const char* baseB = dzi + (ts * H + c) * (int64_t)4096;
    SpAcc acc;
    sp_zero(acc);
    auto dma = [&](int st, int64_t f, int piece) {
        const int q = piece % SP_PW;
        if (piece < SP_PW) {   // E rows past T - 1 re-read row T - 1: their dz rows are the zero pad
            uint32_t tk = tokq[q];
            const int64_t left = T - 1 - (ts + f * SPK);
            if (left < SPK) tk = tk < (uint32_t)left ? tk : (uint32_t)left;
            glds16_s(tk * (uint32_t)e_rsb + coA[q], sp_uniform(baseA + f * SPK * e_rsb), lds_addr_of(&sm3.A[st][(wave * SP_PW + q) * 1024]));
        } else {
            glds16_s(tokq[q] * rowB + coB[q], sp_uniform(baseB + f * SPK * (int64_t)rowB), lds_addr_of(&sm3.B[st][(wave * SP_PW + q) * 1024]));
        }
    };
    if constexpr (NA == 3) sp_tn_mainloop3<TERMS>(sm3, acc, nch, wm, wn, lane, dma);
    else sp_tn_mainloop<TERMS>(sm3, acc, nch, wm, wn, lane, dma);
    const float inv = 1.f / (e_sc[0] * dz_sc[0]);
    float* so = slabW + (((int64_t)sp * H + c) * HID + i0) * 1024 + n0;
    auto emit = [&](int row, int col, const f32x4& v) { *reinterpret_cast<f32x4*>(so + (int64_t)row * 1024 + col) = v * inv; };
    sp_epilogue_rows<true>(acc, sm, wave, wm, wn, lane, SPM, emit);
}

// ================================================================================================
// host side (gate_host.hpp: the records, the checks, the dispatch and the phases of the backward)
// ================================================================================================
// split_gemm.hip
int sp_launch_absmax(const float* X, int64_t ldx, int64_t rows, int K, float* out, hipStream_t s);
int sp_launch_absmax_flat(const float* x, int64_t n, float* out, hipStream_t s);
int sp_launch_scale(float* sc, hipStream_t s);

// token rows per workgroup of the dz pass: a workgroup walks its rows two at a time (~1.3 us per pair of rows, latency), so 256 rows
// only pay when there are thousands of workgroups to overlap them; a 2,048-token step (config 1) spent 340 us in 8 workgroups
#ifndef MDL_DZ_ROWS_BIG
#define MDL_DZ_ROWS_BIG DZ_ROWS
#endif
static inline int sp_dz_rows(int64_t T) { return T >= 131072 ? MDL_DZ_ROWS_BIG : (T >= 16384 ? 64 : 16); }
// persistent workgroups of the forward (round 5, see sp_gate_fwd_kernel): MADELEINE_GATE_PERSIST = 0 | 1 | 2 picks the mode (A/B switch),
// kept only where gate_persist_pays
static inline int sp_gate_fwd_pmode(int64_t T, int H) {
    return gate_pmode((int)sw(MDL_SW_GATE_PERSIST), T, H, SPM, 0.96, GATE_PT);
}

static GateFwdGeom fwd_geom(int64_t T, int H) { return gate_fwd_grid(T, H, SPM, sp_gate_fwd_pmode(T, H), GATE_PT); }
// dW: 2 x 4 tiles per head and split, one workgroup per CU; + SPK zero rows behind dz
static GateBwdGeom bwd_geom(int64_t T, int H) {
    GateBwdGeom g{};
    g.S = splits_for(T, 8 * H, 256), g.chunk = g.pad = SPK, g.min_chunks = 1, g.dz_rows = sp_dz_rows(T);
    g.dx_tile = SPM, g.dw_tile = 256, g.dw_per = 8;
    return gate_bwd_grid(g, T, H);
}
// scale floats: [0,1] W scale / absmax | [2,3] max|ds|, max|wc| | [4,5] dz scale / bound
static GateFwdWs fwd_ws(int64_t T, int H) { return gate_fwd_ws(T, H, 4, 64); }                      // WK image [H][1024][512]
static GateBwdWs bwd_ws(int64_t T, int H) { return gate_bwd_ws(T, H, bwd_geom(T, H), 4, 4, 64); }   // WN and dz as images
static const GateEngine ENGINE = {
    /*image*/ true, /*elem_bytes*/ 1, /*stride_unit*/ 16, /*head_units*/ HID * 4,
    {SPM, 0},   // fwd: ra * e_rsb + ch * 16, ra < SPM, ch * 16 < e_rsb
    {SPK, 0},   // bwd: the dW kernel's tk * e_rsb + coA, tk < SPK, coA < e_rsb
    /*max_phases*/ 15,
    [](int64_t T, int H) { return gate_fwd_grid(T, H, SPM, 0, 1).grid; },   // a workgroup per tile: never fewer than the persistent grids
    [](int64_t T, int H, int phases) { return gate_bwd_max_grid(bwd_geom(T, H), H, phases); },
};

// the weights' scale from their exact absmax: sc[1] = max |Wa|, |Wb| -> sc[0] (sc zeroed by the caller)
static int sp_weight_scale(const GateParams& p, int H, float* sc, hipStream_t s) {
    if (const int rc = sp_launch_absmax(p.Wa, HID, (int64_t)H * HID, HID, sc + 1, s)) return rc;
    if (const int rc = sp_launch_absmax(p.Wb, HID, (int64_t)H * HID, HID, sc + 1, s)) return rc;
    return sp_launch_scale(sc, s);
}

static int gate_fwd(const GateFwdCall& c) {
    bool empty;
    if (const int rc = gate_check_fwd(ENGINE, c, &empty)) return rc;
    if (empty) return MDL_OK;
    const int64_t T = c.pb.T;
    const int H = c.pb.H;
    const GateParams& p = c.par;
    const DropCfg d = make_drop(c.drop);
    const GateFwdGeom g = fwd_geom(T, H);
    const GateFwdWs L = fwd_ws(T, H);
    char* WK = (char*)c.ws + L.oW;
    float* part = (float*)((char*)c.ws + L.opart);
    float* sc = (float*)((char*)c.ws + L.osc);
    if (const int rc = (int)hipMemsetAsync(sc, 0, 2 * sizeof(float), c.s)) return rc;
    if (const int rc = sp_weight_scale(p, H, sc, c.s)) return rc;
    if (const int rc = gate_launch(sp_gate_wk_kernel, dim3((unsigned)((int64_t)H * 1024 * 64 / 256)), 256, c.s, p.Wa, p.Wb, WK, H, sc)) return rc;
    // <PMODE, NA>: the persistent modes exist with two stages only, the three-stage ring (sp_nt_mainloop3, MADELEINE_SP_NT_STAGES) with
    // one tile per workgroup only
    const int variant = g.pmode ? g.pmode : (sp_nt_stages() == 3 ? 3 : 0);
    const int rc = gate_pick_fwd(d, c.act.a != nullptr, [&](auto dm, auto save) {
        return gate_pick<1, 2, 3, 0>(variant, [&](auto v) {
            constexpr int PM = decltype(v)::value == 3 ? 0 : decltype(v)::value, NA = decltype(v)::value == 3 ? 3 : 2;
            return gate_launch(sp_gate_fwd_kernel<decltype(dm)::value, decltype(save)::value != 0, PM, NA>, dim3((unsigned)g.grid), SP_THREADS,
                               c.s, c.src.p, c.src.ld, c.src.scale, WK, sc, p.ba, p.bb, p.wc, part, c.act.a, c.act.b, T, H, g.n_tt, d);
        });
    });
    if (rc) return rc;
    return gate_launch_finalize(part, p.bc, c.scores, T * H, H, c.s);
}

static int gate_bwd(const GateBwdCall& c) {
    if (const int rc = gate_check_bwd(ENGINE, c)) return rc;
    const int64_t T = c.pb.T;
    const int H = c.pb.H;
    const GateParams& p = c.par;
    const DropCfg d = make_drop(c.drop);
    const GateBwdGeom g = bwd_geom(T, H);
    const GateBwdWs L = bwd_ws(T, H);
    char* base = (char*)c.ws;
    char* WN = base + L.oWN;
    char* dzi = base + L.odz;
    float* slabW = (float*)(base + L.oslabW);
    float* slabV = (float*)(base + L.oslabV);
    float* sc = (float*)(base + L.osc);
    return gate_bwd_phases(
        c, g, slabW, slabV,
        [&] {   // scales: weights from their exact absmax; dz from the bound |dz| <= max|ds| max|wc| / (1-p)^2
            if (const int rc = (int)hipMemsetAsync(sc, 0, 8 * sizeof(float), c.s)) return rc;
            if (const int rc = gate_zero_pad_rows(dzi, T, H, g, 4, c.s)) return rc;
            if (const int rc = sp_weight_scale(p, H, sc, c.s)) return rc;
            if (const int rc = sp_launch_absmax_flat(c.d_scores, T * H, sc + 2, c.s)) return rc;
            if (const int rc = sp_launch_absmax_flat(p.wc, (int64_t)H * HID, sc + 3, c.s)) return rc;
            return gate_launch(sp_bound_scale_kernel, dim3(1), 1, c.s, sc + 2, d.inv * d.inv, sc + 4);
        },
        [&] {
            return gate_pick_dm(d, [&](auto dm) {
                return gate_launch(sp_gate_dz_kernel<decltype(dm)::value>, dim3((unsigned)g.nblk), 64 * H, c.s, p.wc, c.act.a, c.act.b, c.d_scores,
                                   dzi, sc + 4, slabV, T, H, d, g.dz_rows);
            });
        },
        [&] {
            if (const int rc = gate_launch(sp_gate_wn_kernel, dim3(16, 32, H), 256, c.s, p.Wa, p.Wb, WN, sc)) return rc;
            return gate_pick<2, 3>(c.pb.terms, [&](auto terms) {
                return gate_pick<3, 2>(sp_nt_stages(), [&](auto na) {
                    return gate_launch(sp_gate_dx_kernel<decltype(terms)::value, decltype(na)::value>, dim3((unsigned)g.dx_grid), SP_THREADS, c.s,
                                       dzi, sc + 4, WN, sc, c.de.p, c.de.ld, c.de.accumulate, T, H, c.pt, c.de.absmax);
                });
            });
        },
        [&] {
            return gate_pick<2, 3>(c.pb.terms, [&](auto terms) {
                return gate_pick<3, 2>(sp_tn_stages(), [&](auto na) {
                    return gate_launch(sp_gate_dw_kernel<decltype(terms)::value, decltype(na)::value>, dim3((unsigned)g.dw_grid), SP_THREADS, c.s,
                                       c.src.p, c.src.ld, c.src.scale, dzi, sc + 4, slabW, T, H, g.tps, g.S);
                });
            });
        });
}

}  // namespace mdl

using namespace mdl;

extern "C" int64_t mdl_abmil_gate_fwd_split_ws_bytes(int64_t T, int H) { return gate_ws_bytes(T, H, fwd_ws); }

/* mdl_abmil_gate_fwd on the split engine: E as a split image (rows of e_rsb bytes holding the H*512 head-major channels, scale e_scale);
 * everything else as mdl_abmil_gate_fwd (fp32 parameters, scores, saved activations). */
extern "C" int mdl_abmil_gate_fwd_split(const void* E_img, int64_t e_rsb, const float* e_scale, const float* Wa, const float* ba,
                                        const float* Wb, const float* bb, const float* wc, const float* bc, float* scores, float* act_a,
                                        float* act_b, int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a,
                                        const uint8_t* keep_b, void* ws, void* stream) {
    return gate_fwd({{E_img, e_rsb, e_scale}, {Wa, ba, Wb, bb, wc, bc}, scores, {act_a, act_b}, {p_drop, seed, keep_a, keep_b}, {T, H, 3, 3},
                     ws, (hipStream_t)stream});
}

extern "C" int64_t mdl_abmil_gate_bwd_split_ws_bytes(int64_t T, int H) { return gate_ws_bytes(T, H, bwd_ws); }

/* mdl_abmil_attnpool_bwd (scores == NULL: plain mdl_abmil_gate_bwd) on the split engine; E as a split image.  dE_absmax (device float,
 * may be NULL; zeroed by the caller) is raised to max |dE|.  phases: bit 0 as mdl_abmil_attnpool_bwd_phases, bit 1 = both contractions,
 * bit 2 = dX only, bit 3 = dW only. */
extern "C" int mdl_abmil_attnpool_bwd_split(const void* E_img, int64_t e_rsb, const float* e_scale, const float* Wa, const float* Wb,
                                            const float* wc, const float* act_a, const float* act_b, const float* d_scores, float* dE,
                                            int64_t ldE, int accumulate, float* dWa, float* dWb, float* dba, float* dbb, float* dwc,
                                            float* dbc, int64_t T, int H, float p_drop, uint64_t seed, const uint8_t* keep_a,
                                            const uint8_t* keep_b, const float* scores, const float* stat_m, const float* stat_l,
                                            const float* d_pooled, const int32_t* row_bag, int64_t N, float* dE_absmax, void* ws,
                                            void* stream, int phases, int terms) {
    return gate_bwd({{E_img, e_rsb, e_scale}, {Wa, nullptr, Wb, nullptr, wc, nullptr}, {act_a, act_b}, d_scores,
                     {dE, ldE, accumulate, dE_absmax}, {dWa, dWb, dba, dbb, dwc, dbc}, {p_drop, seed, keep_a, keep_b},
                     {scores, stat_m, stat_l, d_pooled, row_bag, N}, false, {T, H, phases, terms}, ws, (hipStream_t)stream});
}

namespace mdl {
// mdl_dispatch_plan (dispatch_plan.hip): the forward's persistence mode and the token splits of the backward's dW contraction
int plan_gate_split(int product, int64_t T, int H, int64_t* o) {
    if (!gate_heads_ok(H)) return MDL_E_UNSUPPORTED;
    if (product == MDL_PLAN_GATE_SPLIT_FWD) {
        o[MDL_PLAN_PERSIST] = fwd_geom(T, H).pmode;
        o[MDL_PLAN_SPLITS] = 1;
        return MDL_OK;
    }
    plan_splits(o, T, bwd_geom(T, H));
    return MDL_OK;
}
}  // namespace mdl
