// Host-side sequencing of the LA-VAE decoder (LADiffVae.decode, ladiff_vae.py:288-362) on the gfx950 kernels.
// Activations are kept batch-major [B*F, 256] (the reference is [F, B, 256]); all ops are per-row or per-sample,
// so this only changes strides and lets the final write land directly in [B, F, C].
#include "model.h"

namespace ladiff {

// Diagnostic twin only: LADIFF_DEC_CUT=n in the environment (read per call) ends a decode after its first n launches (garbage output) -
// scripts/two_streams_aggressor_bisect.py bisects with it which launch of a co-running decode disturbs another one.  Nothing of it is in the product.
#ifdef LADIFF_STAMPS
#define DEC_CUT() do { if (dec_cut >= 0 && ++dec_launched >= dec_cut) { dec_done = true; return 0; } } while (0)
#define DEC_STEP(step) do { LADIFF_TRY(step); if (dec_done) return 0; } while (0)      // a cut inside a layer step ends the decode
#else
#define DEC_CUT() do { } while (0)
#define DEC_STEP(step) LADIFF_TRY(step)
#endif

DecSwitchAtoms g_dec;                          // the measurement switches (model.h); a decode runs on its caller's snapshot `sw`

// wsp != nullptr selects the f16x3 matrix path (S-format copies of the weight matrices in `wsp`, GEMM operands in
// S-format, LayerNorm as a row kernel after each fused GEMM); see denoiser.hip and common.h.
// row_off != nullptr (B + 1 entries, row_off[B] = R): RAGGED rows - sample b owns rows [row_off[b], row_off[b] + lengths[b]) and
// only the R valid frames of a mixed-length batch are computed.  Every op of the decoder is per row or per sample (padded
// frames are masked keys, cross_attention.py:367-371, and zeroed at the end, ladiff_vae.py:356-360), so a sample's frames come
// out as in the padded layout; they are scattered to feats[b, f < length] of a [B, F, C] tensor the caller has zero-filled.
//
// Launches: 2 up front (K | V batch, cross prep), the position rows, nine layers, final_layer.  Per layer, by DecRoute (graph_key.h):
//   fp32 (6)            in_proj gemm | self-attention | out_proj gemm (+ residual + norm1 in its epilogue) | cross_apply (+ norm2) | linear1 gemm |
//                       linear2 gemm (+ residual + norm3 [+ decoder.norm] in its epilogue)
//   f16x3 small (7)     in_proj gemm_kr | self-attention (split) | out_proj gemm_kr (+ residual) | cross_apply (norm1 as it loads) | linear1 gemm_kr |
//                       linear2 gemm_kr (four K planes) | reduce_rows (sum + residual + norm3 [+ decoder.norm])
//   f16x3 large-M (5)   dec_qkv_attn (in_proj inside) | out_cross (out_proj .. norm2) | linear1 gemm | linear2 gemm (+ residual) | reduce_rows
//                       (norm3 [+ decoder.norm]);  from dec_mlp_min_rows() rows (3): dec_mlp instead of the last three; where out_cross
//                       and dec_mlp both run (2): dec_post instead of the two (out_proj .. norm3 in one kernel), + 1 launch up front
//                       (dec_post_gu: every layer's U transposed in place)
//   layer 0: in_proj once on the F position rows (broadcast_pe + gemm / gemm_kr), never inside the attention kernel.  Output blocks (+ 1): the
//   skip concat first (gemm; small: gemm_rowln).  Switches - small_rows_path 0: the large-M forms at any row count;  fused_attn 0: in_proj gemm +
//   self-attention (split), 2: dec_qkv_attn below 4,096 rows too;  out_cross 0: out_proj gemm + cross_apply;  fused_mlp 0: never dec_mlp, 2: always;
//   final_split 0: final_layer on the fp32 gemm as in fp32 mode, else pad_rows + gemm + scatter_feats;  post_off 1: never dec_post
// att_maps != nullptr ([NL][B][F][T], layers in execution order): out_cross off for this call, and cross_maps (+ 1 per layer) between the
//   out_proj gemm and cross_apply.  A call without it makes the launches above.
int vae_decode(const DecoderW& w, const DecoderW* wsp, const float* z, const int32_t* lengths, const int32_t* counts,
               const int32_t* row_off, int R, int B, int F, int T, int C, float* feats, float* ws, size_t ws_floats, hipStream_t s, const DecSwitches& sw,
               float* att_maps) {
    if (F < 1 || F > LADIFF_MAX_FRAMES || T < 1 || T > LADIFF_MAX_LATENTS || C < 1) return LADIFF_ERR_SHAPE;
    const bool ragged = row_off != nullptr;
    if (ragged && (R < 0 || (size_t)R > (size_t)B * F)) return LADIFF_ERR_SHAPE;
    const int M = ragged ? R : B * F;
    DecWs a = dec_layout(ws, B, (size_t)M, T);
    if (ws_floats < a.total) return LADIFF_ERR_WORKSPACE;
    if (M == 0) return 0;
#ifdef LADIFF_STAMPS
    const char* dec_cut_env = getenv("LADIFF_DEC_CUT");
    const int dec_cut = dec_cut_env ? atoi(dec_cut_env) : -1;
    int dec_launched = 0; bool dec_done = false;
    if (dec_cut == 0) return 0;
#endif
    const bool sp = wsp != nullptr;
    // Few frame rows (config c1: 8 x 60 = 480): a 128x128-tile launch is then 8 - 32 workgroups that each walk the whole K, ~16 us per
    // GEMM whatever its size (profiles/r3: 40 of them were 0.63 of a 0.9 ms decode).  Below DEC_SMALL_ROWS the f16x3 path runs its
    // GEMMs on the denoiser's small-M kernels instead (gemm_kr.hip: K-resident 32 / 64 / 80-row tiles, K = 1024 as four partial planes
    // that the LayerNorm row pass sums) - the same S-format operands and products, 3 - 4x the workgroups.  From DEC_SMALL_ROWS up in_proj
    // runs inside the attention kernel (dec_qkv_attn.hip; 8 x 60 frames: 0.47 ms against 0.45 with the small-M in_proj + attention
    // launches; 128 x 196: 2.28 against 2.41, profiles/r3/15).
    // att_maps: the weights are taken from the rows cross_apply reads, which the fused out_proj + cross kernel never writes - such a call
    // routes as one with that kernel switched off (every other switch as the caller's)
    DecSwitches swr = sw;
    if (att_maps != nullptr) swr.out_cross = 0;
    const DecRoute rt = dec_route(sp, M, swr, dec_mlp_min_rows());
    const Seq c{sp, M, s};
    const DecoderW& wm = mfma_table(w, wsp);
    Twin P[4], SK[NSKIP];
    pair_up(sp, a.P, a.Ps, P); pair_up(sp, a.SK, a.SKs, SK);
    const Twin pex = pair(sp, a.pex, a.pexs), att_x = operand_only(sp, a.att), hid_x = operand_only(sp, a.hid);
    float *qkv = a.qkv, *att = a.att, *hid = a.hid, *kv = a.kv, *guws = a.guws, *qkv0 = a.qkv0;

    // The memory side of every layer's cross-attention depends on z and the weights only: the nine K | V projections and the
    // nine folds into G | U | c run up front, one launch each (fp32 in both modes).   cross_attention.py:373-376
    {
        GemmArgs g[NL];
        DecCrossPrepBatch pb;
        for (int l = 0; l < NL; ++l) {
            const DecLayerW& L = w.layer[l];
            g[l] = lin(z, D, L.cross_attn.in_w + (size_t)D * D, L.cross_attn.in_b + D, kv + l * a.kv_layer, 2 * D, T * B, 2 * D, D);
            pb.kv[l] = kv + l * a.kv_layer; pb.wq[l] = L.cross_attn.in_w; pb.bq[l] = L.cross_attn.in_b; pb.wo[l] = L.cross_attn.out_w;
            pb.gu[l] = guws + l * a.gu_layer;
        }
        LADIFF_TRY(launch_gemm_batch(g, NL, s)); DEC_CUT();
        LADIFF_TRY(launch_decoder_cross_prep(pb, NL, B, T, s)); DEC_CUT();
        // the one-kernel layer tail reads U transposed: every layer's U rows re-laid in place, one launch (dec_post.hip)
        if (rt.post) { LADIFF_TRY(launch_dec_post_gu(guws, a.gu_layer, NL, B, T, s)); DEC_CUT(); }
    }

    // a projection of the small route over `rows` rows (gemm_kr.hip; the route exists in f16x3 mode only)
    auto krs = [&](Twin x, int K, const LinearW& W, Twin y, int ldy, int N, int act, const float* res, int rows) -> int {
        KrArgs g = proj_kr(Seq{sp, rows, s}, x, K, W, y, ldy, N, act, res);
        g.ldres = D;
        return launch_gemm_kr(g, s);
    };
    int l = 0; DecLayerW L; Twin cur = P[0];      // the layer, its weights as the mode reads them (seq.h), its input: what the four steps work on

    // x = linear(cat([x, xs.pop()]))   cross_attention.py:140-142
    // small: whole 256-wide rows per workgroup, K = 512 streamed (gemm_rowln.hip, as the denoiser's skip layers)
    auto skip_concat = [&]() -> int {
        const LinearW sk = mixed(w.skip[l - NSKIP - 1], wm.skip[l - NSKIP - 1]);
        LADIFF_TRY(rt.small ? skip_rowln(c, cur, SK[NL - 1 - l], sk, P[3]) : skip_gemm(c, cur, SK[NL - 1 - l], sk, P[3])); DEC_CUT();
        cur = P[3];
        return 0;
    };

    // self-attention over frames, keys >= len masked   cross_attention.py:367-371
    // Layer 0's input is the position table for every sample (queries = zeros + pe, ladiff_vae.py:299, :334): its in_proj runs on
    // the F table rows once and every sample's attention reads those q | k | v (its own length still masks the keys).
    auto self_attention = [&]() -> int {
        const LinearW in = in_proj(L.self_attn);
        const bool shared = l == 0; const Twin q = {shared ? qkv0 : qkv, nullptr};
        if (shared) {
            LADIFF_TRY(launch_broadcast_pe(w.query_pe, 1, F, pex.f, pex.s, s)); DEC_CUT();
            if (rt.small) { LADIFF_TRY(krs(pex, D, in, q, 3 * D, 3 * D, ACT_NONE, nullptr, F)); DEC_CUT(); }
            else { LADIFF_TRY(launch_gemm(proj(Seq{sp, F, s}, pex, D, in, q, 3 * D, 3 * D), s)); DEC_CUT(); }
        } else if (rt.fused_attn) {      // in_proj inside the attention kernel (dec_qkv_attn.hip) - the [M, 768] q | k | v rows are never written
            LADIFF_TRY(launch_dec_qkv_attn(cur.s, in.w, in.b, lengths, row_off, att, B, F, 1, s)); DEC_CUT();
            return 0;
        } else if (rt.small) { LADIFF_TRY(krs(cur, D, in, q, 3 * D, 3 * D, ACT_NONE, nullptr, M)); DEC_CUT(); }
        else { LADIFF_TRY(launch_gemm(proj(c, cur, D, in, q, 3 * D, 3 * D), s)); DEC_CUT(); }
        if (sp) { LADIFF_TRY(launch_self_attention_split(q.f, lengths, nullptr, att, B, F, H, 0, 1, s, row_off, shared)); DEC_CUT(); }
        else { LADIFF_TRY(launch_decoder_self_attention(q.f, lengths, nullptr, att, B, F, 0, s, row_off, shared)); DEC_CUT(); }
        return 0;
    };

    // x + out_proj(att), norm1, cross-attention to the latent tokens (tokens >= ceil(len/48) masked) + residual + norm2 -> P[2]   :373-376, :408-409
    // (the q / out projections of the cross-attention are folded into the <= 8 keys / values per sample: dec_cross.hip; fp32 in both modes)
    auto out_proj_cross_attention = [&]() -> int {
        const LinearW out = out_proj(L.self_attn); float* gu = guws + l * a.gu_layer;
        if (rt.out_cross) {
            // f16x3 mode, many rows: out_proj + residual + norm1 + cross-attention + residual + norm2 in ONE kernel that keeps Wo in
            // its registers (dec_cross.hip): x + out_proj(att) is never written
            LADIFF_TRY(launch_decoder_out_cross(att, cur.f, out.w, out.b, L.norm1.g, L.norm1.b, L.cross_attn.out_b, L.norm2.g, L.norm2.b,
                                                counts, B, F, T, gu, P[2].f, P[2].s, s, row_off)); DEC_CUT();
            return 0;
        }
        // norm1: fused in the GEMM epilogue in fp32 mode; in f16x3 mode the GEMM writes x + out_proj(att) and the only reader of
        // norm1's output, the cross-attention kernel, normalises its rows as it loads them (one row kernel pass less)
        const Twin r1 = {P[1].f, nullptr};
        if (rt.small) { LADIFF_TRY(krs(att_x, D, out, r1, D, D, ACT_NONE, cur.f, M)); DEC_CUT(); }
        else if (sp) { LADIFF_TRY(launch_gemm(proj(c, att_x, D, out, r1, D, D, ACT_NONE, cur.f), s)); DEC_CUT(); }
        else { LADIFF_TRY(gemm_ln(c, att_x, D, out, cur.f, L.norm1, nullptr, r1, true)); DEC_CUT(); }
        const NormW n1_late = sp ? L.norm1 : NormW{nullptr, nullptr};
        if (att_maps != nullptr) {      // the layer's map [B][F][T] from the same rows, folded keys and counts (dec_cross.hip)
            LADIFF_TRY(launch_decoder_cross_maps(P[1].f, counts, lengths, B, F, T, gu, att_maps + (size_t)l * B * F * T, s, row_off, n1_late.g,
                                                 n1_late.b)); DEC_CUT();
        }
        LADIFF_TRY(launch_decoder_cross_apply(P[1].f, L.cross_attn.out_b, L.norm2.g, L.norm2.b, counts, B, F, T, gu, P[2].f, P[2].s, s, row_off,
                                              n1_late.g, n1_late.b)); DEC_CUT();
        return 0;
    };

    // feed-forward, GELU(erf), + residual + norm3 (+ decoder.norm on the last layer, cross_attention.py:150-151) -> dst   :410-412
    auto feed_forward = [&](Twin dst) -> int {
        const NormW* fin = l == NL - 1 ? &w.norm : nullptr;
        if (rt.fused_mlp) {             // one kernel: the hidden rows never leave the registers (dec_mlp.hip)
            LADIFF_TRY(launch_dec_mlp(P[2].s, P[2].f, L.lin1.w, L.lin1.b, L.lin2.w, L.lin2.b, L.norm3.g, L.norm3.b, fin ? fin->g : nullptr,
                                      fin ? fin->b : nullptr, dst.f, dst.s, M, s, sw.mlp_variant)); DEC_CUT();
        } else if (rt.small) {
            LADIFF_TRY(krs(P[2], D, L.lin1, hid_x, FF, FF, ACT_GELU, nullptr, M)); DEC_CUT();
            // linear2: K = 1024 as four partial planes (the q|k|v + attention buffers are free by now), summed by the LayerNorm pass
            LADIFF_TRY(krs(hid_x, FF, LinearW{L.lin2.w, nullptr}, Twin{qkv, nullptr}, D, D, ACT_NONE, nullptr, M)); DEC_CUT();
            RedArgs r = red(c, qkv, 4, L.lin2.b, P[2].f, &L.norm3, dst);
            if (fin) { r.g2 = fin->g; r.b2 = fin->b; }
            LADIFF_TRY(launch_reduce_rows(r, s));
        } else {
            LADIFF_TRY(launch_gemm(proj(c, P[2], D, L.lin1, hid_x, FF, FF, ACT_GELU), s)); DEC_CUT();
            LADIFF_TRY(gemm_ln(c, hid_x, FF, L.lin2, P[2].f, L.norm3, fin, dst, true)); DEC_CUT();      // norm3, then decoder.norm: one row pass
        }
        return 0;
    };

    // the two steps above as ONE launch (dec_post.hip): x0 + out_proj(att), norm1's output and the feed-forward input are never written
    auto post_attention = [&](Twin dst) -> int {
        const LinearW out = out_proj(L.self_attn); const float* gu = guws + l * a.gu_layer;
        const NormW* fin = l == NL - 1 ? &w.norm : nullptr;
        const DecPostArgs pa{att, cur.f, out.w, out.b, L.norm1.g, L.norm1.b, gu, gu + (size_t)B * H * T * 2 * D, L.cross_attn.out_b, L.norm2.g,
                             L.norm2.b, counts, row_off, L.lin1.w, L.lin1.b, L.lin2.w, L.lin2.b, L.norm3.g, L.norm3.b,
                             fin ? fin->g : nullptr, fin ? fin->b : nullptr, dst.f, dst.s, B, F, T, M};
        LADIFF_TRY(launch_dec_post(pa, s)); DEC_CUT();
        return 0;
    };

    // queries = zeros + query_pos_decoder.pe[:F]     ladiff_vae.py:299, :334
    if (ragged) { LADIFF_TRY(launch_broadcast_pe_ragged(w.query_pe, row_off, B, F, F, P[0].f, P[0].s, a.row_out, s)); DEC_CUT(); }
    else { LADIFF_TRY(launch_broadcast_pe(w.query_pe, B, F, P[0].f, P[0].s, s)); DEC_CUT(); }
    for (l = 0; l < NL; ++l) {          // SkipTransformerDecoder: four input blocks push, the four output blocks pop   cross_attention.py:128-151
        L = mixed(w.layer[l], wm.layer[l]);
        if (l > NSKIP) DEC_STEP(skip_concat());
        DEC_STEP(self_attention());
        const Twin dst = l < NSKIP ? SK[l] : P[0];
        if (rt.post) DEC_STEP(post_attention(dst));
        else {
            DEC_STEP(out_proj_cross_attention());
            DEC_STEP(feed_forward(dst));
        }
        cur = dst;
    }
    // final_layer + zero padded frames, written as [B, F, C]   ladiff_vae.py:356-360
    if (rt.final_split) {
        // f16x3 mode: the projection runs on the large-M f16x3 kernel over whole 128-column tiles, into the (free) hidden buffer, and a
        // row kernel moves the C real columns into [B, F, C] (zeroing padded frames / scattering ragged rows): 94 us -> ~40 us at 25088
        // rows.  The tiles need Np = ceil(C / 128) 128 weight rows: the library pads the caller's C rows ITSELF (a 1-KiB-per-row copy
        // into the in_proj buffer, free by now) - a table of exactly C rows is never read past its end.
        const int Np = (C + 127) / 128 * 128;
        if ((size_t)M * Np > a.hid_floats || (size_t)Np * (D + 1) > a.qkv_floats) return LADIFF_ERR_SHAPE;      // the two buffers it re-uses
        float* wpad = qkv; float* bpad = qkv + (size_t)Np * D;
        LADIFF_TRY(launch_pad_rows(wm.final_layer.w, w.final_layer.b, wpad, bpad, C, Np, s)); DEC_CUT();
        LADIFF_TRY(launch_gemm(proj(c, cur, D, LinearW{wpad, bpad}, Twin{hid, nullptr}, Np, Np), s)); DEC_CUT();
        return launch_scatter_feats(hid, Np, C, M, F, ragged ? nullptr : lengths, ragged ? a.row_out : nullptr, feats, s);
    }
    GemmArgs g = lin(cur.f, D, w.final_layer, feats, C, M, C, D);
    if (ragged) g.row_map = a.row_out;                      // every computed row is a valid frame
    else { g.row_len = lengths; g.rows_per_item = F; }
    return launch_gemm(g, s);
}

}  // namespace ladiff
