"""fq_stage_ref.py -- TEST INFRASTRUCTURE: the transform-and-quantise kernels of th_encode_* (the plain ones, their block-qi forms and
their masked forms) as thip_enc_fq_stage (include/theora_hip.h) hands their results out.  Nothing is restated here: the source, the
prediction and the residual are inter_stage_ref's, the transform and the quantiser the oracle's, the AC bits enc_bqi_ref's, the block's
lambda and the choice rule enc_skip_ref's (without its skip test); this module composes them over given arrays.

Everything is in bitstream coordinates, as in inter_stage_ref.  Besides what the kernels write, stage() returns what they choose from
and do not hand out -- every block's D_k, R_k and lambda_b and its levels at every qi of the list -- so that a test can assert that
a case reaches its edge.  Python ints wherever a product may pass 32 bits: D_k + lambda_b R_k is an object array.
"""
import numpy as np

import oracle
from tests import enc_modes_ref as MR
from tests import enc_skip_ref as S
from tests import inter_stage_ref as R
from tests.packref import EXTRA_BITS

NOMV, INTRA = MR.NOMV, MR.INTRA


def code_lengths(bits):
    """The entry's bits (uint8 [2][4][32], code length + extra bits) as enc_bqi_ref.ac_bits takes them, which adds a token's extra
    bits itself: (luma, chroma) [4][32].  (Python ints, and negative where a planted length lies below the extra bits: the sum is the
    entry's byte again.)"""
    return (np.asarray(bits, np.int64).reshape(2, 4, 32) - np.asarray(EXTRA_BITS, np.int64)[None, None, :]).tolist()


def stage(geo, src, classes, nqis, dequant, bits=None, prev=None, gold=None, pix=None, mv=None, bmv=None, iscale=None):
    """thip_enc_fq_stage's outputs and the choice behind them.  src: inter_stage_ref.frame_src's planes; classes 0: a key frame (prev,
    gold and the decisions pix [nmbs], mv [nmbs, 2], bmv [nmbs, 4, 2] unused), 2 / 3: an inter frame; nqis 0: no choice; dequant
    [max(nqis, 1)][2][3][64], with classes 0 [max(nqis, 1)][3][64]; bits uint8 [2][4][32]; iscale [nfrags] or None.
    dict(levels [nfrags, 64] int16 and qii uint8 in CODED order; dcq, cmap, dcr raster (cmap, dcr None with classes 0);
         D, R [nfrags, nqis] and lam [nfrags] in CODED order, Python ints in object arrays (None with nqis 0);
         lev_k [max(nqis, 1)][nfrags, 64]: the levels at each qi of the list, raster; lev, qti, fpix, coded: raster)."""
    nf, K = geo.nfrags, max(nqis, 1)
    if classes == 0:
        fpix = np.full(nf, INTRA, np.int64)
        fvx = fvy = np.zeros(nf, np.int64)
        dq = np.asarray(dequant, np.int64).reshape(K, 1, 3, 64)
        prev = gold = None
    else:
        pix, mv = np.asarray(pix, np.int64), np.asarray(mv, np.int64)
        bmv = np.zeros((len(pix), 4, 2), np.int64) if bmv is None else np.asarray(bmv, np.int64)
        fvx, fvy = MR.fragment_vectors(geo, pix, mv, bmv)
        fpix = pix[geo.mb_of]
        dq = np.asarray(dequant, np.int64).reshape(K, 2, 3, 64)
    dct, qti = R.coefficients_of(geo, src, prev, gold if classes == 3 else None, fpix, fvx, fvy)
    lev = np.zeros((nf, 64), np.int64)
    lev_k = np.zeros((K, nf, 64), np.int64)
    qii = np.zeros(nf, np.int64)
    D, Rk, lam = np.zeros((nf, K), object), np.zeros((nf, K), object), np.zeros(nf, object)
    b2 = code_lengths(bits) if nqis else None
    for f in range(nf):
        p = int(geo.plane_of[f])
        tabs = [dq[k, int(qti[f]), p] for k in range(K)]   # (a key frame's set holds the intra tables alone: qti 0)
        if not nqis:
            lev[f] = lev_k[0, f] = oracle.quantize_batch(dct[f:f + 1], tabs[0].astype(np.uint16))[0][0]
            continue
        cand = S.block_candidates(dct[f], tabs, b2[int(p > 0)])
        lam[f] = S.block_lambda(tabs[0], None if iscale is None else iscale[f])
        k = S.choose_candidate(cand, lam[f])
        for kk, (q, d, r) in enumerate(cand):
            lev_k[kk, f], D[f, kk], Rk[f, kk] = q, d, r
        qii[f] = k
        lev[f] = cand[k][0]
        lev[f, 0] = cand[0][0][0]   # the DC stays at qis[0]
    co = geo.coded_order
    out = dict(levels=lev[co].astype(np.int16), dcq=lev[:, 0].astype(np.int16), qii=qii[co].astype(np.uint8), cmap=None, dcr=None,
               D=D[co] if nqis else None, R=Rk[co] if nqis else None, lam=lam[co] if nqis else None, lev_k=lev_k, lev=lev, qti=qti,
               fpix=fpix, coded=np.ones(nf, bool))
    if classes:
        fgold = (fpix == MR.GOLDEN_NOMV) | (fpix == MR.GOLDEN_MV)
        assert classes == 3 or not fgold.any()
        cls = np.where(qti == 0, 1, np.where(fgold, 3, 2))
        coded = (fpix != NOMV) | (lev != 0).any(1)
        out.update(cmap=(coded * cls).astype(np.uint8), dcr=MR.dc_residuals(geo, lev, coded, cls, classes).astype(np.int16), coded=coded)
    return out
