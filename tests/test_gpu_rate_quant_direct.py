"""The rate probe's k_rate_dc and k_rate_tok under quantiser steps that rise and fall with q, driven directly through
thip_enc_rate_stage with any_order = 1 (include/theora_hip.h), against tests/rate_stage_ref.py, which quantises every block at every
q by itself and so rests on no order of the steps.

The kernels walk the indices whose coefficient is not zero under the FLOOR, the least step over q of each (table, z).  They once
balloted at qi 63; every planted coefficient here is non-zero at one q only and zero at qi 63, so that ballot would have dropped it.
16 x 16 (six blocks: most of a work group idle) and 64 x 48 (72 blocks, more than one work group), key and inter.  Every qdc, ballot
word and partial bin equals the restatement; every output lies in front of a guard that must come back untouched."""
import numpy as np
import pytest

from tests import enc_quant_ref as QR
from tests import enc_ref
from tests import rate_stage_ref as R
from tests.test_gpu_rate_direct import geometry, same, sparse_coef, steps

pytestmark = pytest.mark.gpu

DC, TOK = 2, 4
_GUARD = 64
FRAMES = [(16, 16), (64, 48)]
EDGES = (1, 5, 6, 14, 15, 27, 28, 63)   # the first and last zig-zag index of the Huffman groups' edges
LAM = 20 + 3 * np.arange(64)


def run(frame, inter, stages, st, any_order=1, coef=None, stats=None, qdc=None, coded=None, cls=None, lam=None):
    """thip_enc_rate_stage on a 4:2:0 frame -> dict of what the stages wrote.  Outputs are filled with 0x5A and end in a guard."""
    import torch
    from theora_amd.encoder import rate_groups, rate_stage
    n = geometry(frame[0], frame[1], 0).nfrags
    G = rate_groups(n)
    sizes = dict(qdc=n * 128, coded=n * 8, cls=n * 8, partial=G * 64 * 321 * 4)
    dt = dict(qdc=np.int16, coded=np.uint64, cls=np.uint64, partial=np.uint32)
    shape = dict(qdc=(n, 64), coded=(n,), cls=(n,), partial=(G, 64, 321))
    writes = (({"qdc"} | ({"coded", "cls"} if inter else set())) if stages & DC else set()) | ({"partial"} if stages & TOK else set())
    given = dict(qdc=qdc, coded=coded, cls=cls)
    bufs, kw = {}, {}
    for name in ("coef", "stats"):
        v = dict(coef=(coef, np.int16), stats=(stats, np.uint32))[name]
        if v[0] is not None:
            bufs[name] = torch.from_numpy(np.ascontiguousarray(v[0], v[1]).view(np.uint8).reshape(-1).copy()).cuda()
            kw[name] = bufs[name].data_ptr()
    for name, size in sizes.items():
        if name not in writes and given.get(name) is None:
            continue
        t = torch.full((size + _GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        if name not in writes:
            t[:size] = torch.from_numpy(np.ascontiguousarray(given[name], dt[name]).view(np.uint8).reshape(-1).copy()).cuda()
        bufs[name] = t
        kw[name] = t.data_ptr()
    torch.cuda.synchronize()
    rc = rate_stage(frame, 0, inter, stages, steps=st, lam=lam, any_order=any_order, **kw)
    assert rc == 0, rc
    res = {}
    for name in writes:
        a = bufs[name].cpu().numpy()
        assert (a[sizes[name]:] == 0x5A).all(), "%s: written beyond its end" % name
        res[name] = a[:sizes[name]].view(dt[name]).reshape(shape[name])
    return res


def check(frame, inter, st, coef, stats=None, any_order=1, what=""):
    """DC | TOK in one call, then TOK alone on the restatement's qdc and ballots: everything equals tests/rate_stage_ref.py."""
    from theora_amd.encoder import rate_groups
    geo = geometry(frame[0], frame[1], 0)
    G = rate_groups(geo.nfrags)
    lam = LAM if inter else None
    kept = {}
    qdc, coded, cls = R.dc_stage(geo, coef, st, inter, stats, lam, kept)
    want = R.tok_stage(geo, coef, qdc, coded, cls, st, inter, stats, lam, G, kept)
    got = run(frame, inter, DC | TOK, st, any_order, coef=coef, stats=stats, lam=lam)
    same(got["qdc"], qdc, "k_rate_dc qdc " + what)
    if inter:
        same(got["coded"], coded, "k_rate_dc coded " + what)
        same(got["cls"], cls, "k_rate_dc cls " + what)
    same(got["partial"], want, "k_rate_tok partial " + what)
    alone = run(frame, inter, TOK, st, any_order, coef=coef, stats=stats, lam=lam, qdc=qdc, coded=coded if inter else None,
                cls=cls if inter else None)
    same(alone["partial"], want, "k_rate_tok alone " + what)
    return qdc, coded, cls, want


def spike_steps(q0):
    """Every step 100, but 10 at q0: the floor is column q0 and no other column, qi 63 among them."""
    st = np.full((6, 64, 64), 100, np.uint16)
    st[:, q0, :] = 10
    return st


def planted(n, nvar, var):
    """[nvar][n][64] natural order: block k holds +-20 at zig-zag index EDGES[k mod 8] of residual `var`, and nothing else.  2|c| =
    40: a level of +-4 under a step of 10, zero under 100."""
    c = np.zeros((nvar, n, 64), np.int16)
    k = np.arange(n)
    c[var, k, enc_ref.ZIGZAG[np.array(EDGES)[k % 8]]] = np.where(k & 1, -20, 20)
    return c


def nomv_stats(nmbs):
    """Every macro block NOMV at every q: S0 = Smv = 0 and SI out of reach."""
    z = np.zeros(nmbs, np.int64)
    return R.pack_stats(z, z, np.full(nmbs, 10 ** 6), z + 3, z - 5)


@pytest.mark.parametrize("q0", [0, 20, 62])
@pytest.mark.parametrize("frame", FRAMES, ids=["16x16", "64x48"])
def test_a_coefficient_of_one_q_alone_key(hip, frame, q0):
    """One coefficient a block, at an edge index of a Huffman group, non-zero at q0 alone and zero at qi 63."""
    geo = geometry(frame[0], frame[1], 0)
    coef = planted(geo.nfrags, 1, 0)
    _, _, _, want = check(frame, 0, spike_steps(q0), coef, what="q0 %d" % q0)
    tot = want.sum(0)[:, :320].reshape(64, 2, 5, 32)
    nz = tot[:, :, :, 7:].sum((1, 2, 3))            # tokens that carry a value or a zero run: none where every level is zero
    assert nz[q0] >= geo.nfrags and not nz[np.arange(64) != q0].any()
    starts = tot[q0][:, 1:, 7:].sum((0, 2))         # the planted index 1 starts in group 1, the zero run before the others too
    assert starts[0] > 0
    if geo.nfrags >= 8:
        assert len({R_group(z) for z in EDGES}) == 4


def R_group(z):
    return enc_ref.huff_group(z)


@pytest.mark.parametrize("q0", [0, 20, 62])
@pytest.mark.parametrize("frame", FRAMES, ids=["16x16", "64x48"])
def test_a_nomv_block_coded_at_the_least_step_alone(hip, frame, q0):
    """Inter, every macro block NOMV: a block is coded exactly where a level is not zero -- at q0 alone, the q of the least step."""
    geo = geometry(frame[0], frame[1], 0)
    nmbs = (frame[0] // 16) * (frame[1] // 16)
    coef = planted(geo.nfrags, 3, 1)
    _, coded, cls, want = check(frame, 1, spike_steps(q0), coef, stats=nomv_stats(nmbs), what="NOMV q0 %d" % q0)
    assert (coded == np.uint64(1 << q0)).all() and (cls == np.uint64(2 ** 64 - 1)).all()
    side = want.sum(0)[:, 320]
    assert side[q0] == 3 * nmbs and not side[np.arange(64) != q0].any()


@pytest.mark.parametrize("inter", [0, 1], ids=["key", "inter"])
@pytest.mark.parametrize("frame", FRAMES, ids=["16x16", "64x48"])
def test_tables_constant_in_q(hip, frame, inter):
    """The floor equals every column: each q quantises alike (inter: the modes still move with lambda)."""
    geo = geometry(frame[0], frame[1], 0)
    nmbs = (frame[0] // 16) * (frame[1] // 16)
    t, _, z = np.ogrid[0:6, 0:64, 0:64]
    st = (9 + 2 * t + 3 * (z & 7) + 0 * _).astype(np.uint16)
    assert np.array_equal(QR.floor(st), st[:, 63, :]) and np.array_equal(QR.floor(st), st[:, 0, :])
    coef = sparse_coef(3 if inter else 1, geo.nfrags, 7 + frame[0], density=0.1, scale=60)
    rng = np.random.default_rng(frame[0])
    stats = R.pack_stats(rng.integers(0, 400, nmbs), rng.integers(0, 400, nmbs), rng.integers(0, 900, nmbs), rng.integers(-31, 32, nmbs),
                         rng.integers(-31, 32, nmbs)) if inter else None
    check(frame, inter, st, coef, stats=stats, what="constant")


@pytest.mark.parametrize("inter", [0, 1], ids=["key", "inter"])
@pytest.mark.parametrize("frame", FRAMES, ids=["16x16", "64x48"])
def test_saw_tables(hip, frame, inter):
    """The steps of the `saw` family of tests/enc_quant_ref.py: for most (table, z) the least step is not at qi 63."""
    geo = geometry(frame[0], frame[1], 0)
    nmbs = (frame[0] // 16) * (frame[1] // 16)
    st = QR.steps(QR.saw_family())
    assert (st[:, 63, :] > QR.floor(st)).mean() > 0.5
    coef = sparse_coef(3 if inter else 1, geo.nfrags, 3 + frame[0], density=0.2, scale=40)
    rng = np.random.default_rng(frame[1])
    stats = R.pack_stats(rng.integers(0, 4000, nmbs), rng.integers(0, 4000, nmbs), rng.integers(0, 9000, nmbs), rng.integers(-31, 32, nmbs),
                         rng.integers(-31, 32, nmbs)) if inter else None
    # levels exist that qi 63 would not have balloted
    lev = R.levels_at(geo, coef, st, 2, np.full(geo.nfrags, R.INTRA if not inter else R.NOMV))
    z63 = R.levels_at(geo, coef, st, 63, np.full(geo.nfrags, R.INTRA if not inter else R.NOMV))
    assert ((lev != 0) & (z63 == 0)).any()
    check(frame, inter, st, coef, stats=stats, what="saw")


@pytest.mark.parametrize("inter", [0, 1], ids=["key", "inter"])
def test_builtin_tables_with_the_opt_in(hip, inter):
    """The built-in tables: the floor is column 63, and the results with any_order = 1 are those with any_order = 0."""
    frame = (64, 48)
    geo = geometry(64, 48, 0)
    st = steps("real")
    assert np.array_equal(QR.floor(st), st[:, 63, :])
    coef = sparse_coef(3 if inter else 1, geo.nfrags, 21, density=0.15, scale=200)
    rng = np.random.default_rng(5)
    stats = R.pack_stats(rng.integers(0, 4000, 12), rng.integers(0, 4000, 12), rng.integers(0, 9000, 12), rng.integers(-31, 32, 12),
                         rng.integers(-31, 32, 12)) if inter else None
    a = check(frame, inter, st, coef, stats=stats, any_order=1, what="built-in, on")
    b = check(frame, inter, st, coef, stats=stats, any_order=0, what="built-in, off")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_the_old_call_form_still_refuses(hip):
    """any_order = 0 refuses steps below those of qi 63, as tests/test_rate_stage_cpu.py pins; any_order = 1 takes them."""
    import torch
    from theora_amd import _lib
    from theora_amd.encoder import rate_stage
    n = geometry(16, 16, 0).nfrags
    coef = torch.zeros(n * 64, dtype=torch.int16, device="cuda")
    qdc = torch.zeros(n * 64, dtype=torch.int16, device="cuda")
    st = spike_steps(20)
    assert rate_stage((16, 16), 0, 0, DC, steps=st, coef=coef.data_ptr(), qdc=qdc.data_ptr()) == _lib.EINVAL
    assert rate_stage((16, 16), 0, 0, DC, steps=st, coef=coef.data_ptr(), qdc=qdc.data_ptr(), any_order=2) == _lib.EINVAL
    assert rate_stage((16, 16), 0, 0, DC, steps=st, coef=coef.data_ptr(), qdc=qdc.data_ptr(), any_order=1) == 0
    bad = st.copy()
    bad[3, 7, 9] = 0
    assert rate_stage((16, 16), 0, 0, DC, steps=bad, coef=coef.data_ptr(), qdc=qdc.data_ptr(), any_order=1) == _lib.EINVAL
    bad[3, 7, 9] = 32768
    assert rate_stage((16, 16), 0, 0, DC, steps=bad, coef=coef.data_ptr(), qdc=qdc.data_ptr(), any_order=1) == _lib.EINVAL
