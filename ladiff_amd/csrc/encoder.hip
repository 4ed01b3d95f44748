// Host-side sequencing of the LA-VAE encoder (LADiffVae.encode, ladiff_vae.py:162-286; live branch: pe "mld", MAX_IT > 0,
// LAD, no MLP_DIST / JOINT_DISTRO_FIX; DVAE as an input pass) - SURVEY.md §8f-3, the row next to the sampling path.  It reuses the
// decoder's kernels: large-M GEMMs with fused residual + LayerNorm, the MFMA self-attention core (now with an arbitrary
// key map: the masked latent tokens sit in the middle of the sequence), row kernels.  Sequence = [T mu tokens | T logvar
// tokens | F frames] per sample, batch-major rows (row = b * S + s), S = 2T + F <= 224.
#include "model.h"

namespace ladiff {

int vae_encode(const EncoderW& w, const EncoderW* wsp, const float* features, const int32_t* lengths, const int32_t* counts,
               const float* eps, int B, int F, int T, int C, float* mu, float* sd, float* latent, float* ws,
               size_t ws_floats, hipStream_t s, const int32_t* slot, const float* values, int n_values) {
    const int S = 2 * T + F;
    if (F < 1 || S > LADIFF_MAX_FRAMES || T < 1 || T > LADIFF_MAX_LATENTS || C < 1) return LADIFF_ERR_SHAPE;
    EncWs a = enc_layout(ws, B, F, T, C);
    if (ws_floats < a.total) return LADIFF_ERR_WORKSPACE;
    const int M = B * S;
    if (B == 0) return 0;
    const bool sp = wsp != nullptr;
    const int Cp = pad32(C);
    const Seq c{sp, M, s};
    const EncoderW& wm = mfma_table(w, wsp);
    Twin P[4], SK[NSKIP];
    pair_up(sp, a.P, a.Ps, P); pair_up(sp, a.SK, a.SKs, SK);
    const Twin att = operand_only(sp, a.att), hid = operand_only(sp, a.hid);
    float *qkv = a.qkv, *featp = a.featp, *wskel = a.wskel, *emb = a.emb;

    // x = skel_embedding(features)  (K = nfeats is padded to a multiple of 32 columns)            ladiff_vae.py:182
    // DVAE (slot given): features + add_noise's field, in the same pass                                :136-150, :175-176
    if (slot != nullptr) LADIFF_TRY(launch_dvae_pad_cols(features, slot, values, n_values, featp, B, F, C, Cp, s));
    else LADIFF_TRY(launch_pad_cols(features, featp, B * F, C, Cp, s));
    LADIFF_TRY(launch_pad_cols(w.skel.w, wskel, D, C, Cp, s));
    LADIFF_TRY(launch_gemm(lin(featp, Cp, wskel, w.skel.b, emb, D, B * F, D, Cp), s));
    // xseq = cat(global_motion_token, x) + query_pos_encoder.pe;  key map from lengths / counts       :189-219
    LADIFF_TRY(launch_encoder_assemble(w.motion_token, emb, w.query_pe, lengths, counts, B, F, T, P[0].f, P[0].s, a.keybits, s));

    Twin cur = P[0];
    for (int l = 0; l < NL; ++l) {       // SkipTransformerEncoder, MD_trans == False branch            cross_attention.py:48-67
        const EncLayerW L = mixed(w.layer[l], wm.layer[l]);
        if (l > NSKIP) {
            LADIFF_TRY(skip_gemm(c, cur, SK[NL - 1 - l], mixed(w.skip[l - NSKIP - 1], wm.skip[l - NSKIP - 1]), P[3]));
            cur = P[3];
        }
        // TransformerEncoderLayer.forward_post                                                         cross_attention.py:293-307
        LADIFF_TRY(launch_gemm(proj(c, cur, D, in_proj(L.self_attn), Twin{qkv, nullptr}, 3 * D, 3 * D), s));
        if (sp) LADIFF_TRY(launch_self_attention_split(qkv, nullptr, a.keybits, att.s, B, S, H, 0, 1, s));
        else LADIFF_TRY(launch_decoder_self_attention(qkv, nullptr, a.keybits, att.f, B, S, 0, s));
        LADIFF_TRY(gemm_ln(c, att, D, out_proj(L.self_attn), cur.f, L.norm1, nullptr, P[1], false));
        LADIFF_TRY(launch_gemm(proj(c, P[1], D, L.lin1, hid, FF, FF, ACT_GELU), s));
        // norm2, then encoder.norm on the last layer: in f16x3 mode two row passes (the decoder's one pass: DESIGN §5)
        const Twin dst = l < NSKIP ? SK[l] : P[0];
        LADIFF_TRY(gemm_ln(c, hid, FF, L.lin2, P[1].f, L.norm2, l == NL - 1 ? &w.norm : nullptr, dst, false));
        cur = dst;
    }
    return launch_encoder_finalize(cur.f, eps, counts, B, T, S, mu, sd, latent, s);
}

}  // namespace ladiff
