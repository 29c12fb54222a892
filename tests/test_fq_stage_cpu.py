"""tests/fq_stage_ref.py (what tests/test_gpu_fq_direct.py compares thip_enc_fq_stage with) against the restatements the packets are
pinned to: on the source, decisions, tables and bits of a key frame and of an eight-mode inter frame of enc_bqi_ref.BqiEncoder its
levels and qii are BqiEncoder._code's, and with scales enc_mask_ref.MaskEncoder._code's.  No GPU."""
import functools

import numpy as np

import oracle
from tests import enc_bqi_ref as B
from tests import enc_mask_ref as K
from tests import enc_modes_ref as M
from tests import enc_ref
from tests import enc_skip_ref as S
from tests import fq_stage_ref as F
from tests import inter_stage_ref as R
from tests.enc_ref import ZIGZAG

W, H, FMT, QI, DELTA = 48, 80, 0, 30, 8


@functools.lru_cache(None)
def _setup():
    from theora_amd.encoder import Encoder
    e = Encoder(16, 16, 0, 32)
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


def _recording(cls):
    """cls with every _code call kept: (src, intra, qis, key, what it returned)."""
    class Rec(cls):
        def _code(self, src, pred, intra, qis, key):
            out = super()._code(src, pred, intra, qis, key)
            self.calls.append((src, np.asarray(intra).copy(), list(qis), key, out))
            return out
    return Rec


def _two_frames(enc):
    """A key frame and an eight-mode inter frame through enc; per frame what fq_stage_ref.stage takes and what _code gave."""
    enc.calls = []
    frames = M.sequence("uncover", W, H, FMT, 4, seed=QI + DELTA)[:2]
    geo, setup = enc.geo, enc.setup
    out = []
    for fr in frames:
        key = not out
        ht = enc.hti[key]
        prev = gold = None
        if not key:
            prev = [enc.ost.get_plane(oracle.FRAME_PREV, p).copy() for p in range(3)]
            gold = [enc.ost.get_plane(oracle.FRAME_GOLD, p).copy() for p in range(3)]
        enc.frame(fr, QI)
        src, intra, qis, was_key, (lev, qii, qti) = enc.calls[-1]
        assert was_key == key and len(qis) == 3
        d = {}
        if not key:
            ms = M.motion_search(src[0], prev[0], gold[0], int(setup.qmat(1, 0, QI)[ZIGZAG][1]))
            d = dict(pix=ms["pix"], mv=ms["mv"], bmv=ms["bmv"])
            assert len(set(ms["pix"].tolist())) > 2 and (intra == (ms["pix"][geo.mb_of] == M.INTRA)).all()
        tabs = np.stack([R.tables_qi(setup, q) for q in qis])     # [nqis][2][3][64]
        out.append(dict(src=src, classes=0 if key else 3, dequant=tabs[:, 0] if key else tabs, bits=S.stage_bits(setup, ht), prev=prev,
                        gold=gold, lev=lev, qii=qii, planes=fr, **d))
    return out


def _stage(geo, c, iscale=None):
    return F.stage(geo, c["src"], c["classes"], 3, c["dequant"], c["bits"], c["prev"], c["gold"], c.get("pix"), c.get("mv"), c.get("bmv"),
                   iscale)


def test_the_stage_is_bqi_encoders_code():
    enc = _recording(B.BqiEncoder)(W, H, FMT, (0, 0, W, H), _setup(), 64, 6, DELTA, modes=True)
    geo = enc.geo
    for c in _two_frames(enc):
        got = _stage(geo, c)
        assert np.array_equal(got["lev"], c["lev"]) and np.array_equal(got["qii"], c["qii"][geo.coded_order])
        assert np.array_equal(got["levels"], c["lev"][geo.coded_order]) and np.array_equal(got["dcq"], c["lev"][:, 0])
        assert len(set(c["qii"].tolist())) == 3
        # what stage() hands out besides: the chosen candidate is the least J, and the DC is qis[0]'s
        J = got["D"] + got["lam"][:, None] * (got["R"] + np.array([0, 1, 1]))
        assert (np.argmin(J.astype(np.int64), 1) == got["qii"]).all()
        assert np.array_equal(got["lev"][:, 0], got["lev_k"][0][:, 0])
    enc.close()


def test_the_masked_stage_is_mask_encoders_code():
    enc = _recording(K.MaskEncoder)(W, H, FMT, (0, 0, W, H), _setup(), 64, 6, DELTA, 4, modes=True)
    geo = enc.geo
    differs = 0
    for c in _two_frames(enc):
        iscale = K.scales(K.activity(c["planes"], W, H, FMT, (0, 0, W, H)), 4, geo)[0]
        assert iscale.min() < 2048 < iscale.max()
        got = _stage(geo, c, iscale)
        assert np.array_equal(got["lev"], c["lev"]) and np.array_equal(got["qii"], c["qii"][geo.coded_order])
        differs += int((_stage(geo, c)["qii"] != got["qii"]).sum())
    assert differs > 0   # (the scales moved a choice: the comparison above is not the unmasked one again)
    enc.close()
