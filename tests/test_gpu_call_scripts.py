"""th_decode_* call sequences on the device against the reference decoder (tests/callscript.py): the same script of calls -- seeks,
th_decode_ctl between frames, dropped frames, a picture asked for twice or not at all -- through oracle.ref.RefDecoder and through
ours, and every return code, granule position, picture and stripe callback of the two transcripts equal.

What the scripts aim at is the interval in which a frame is HELD: with option fe_pipeline (the default) th_decode_ycbcr_out(N) may
have decoded the announced frame N + 1 already, and until the next th_decode_packetin the context's counters, frame type, qi tables
and reference ring belong to a frame the caller has not handed in.  A th_decode_ctl in that interval must behave as if N were the
newest frame (include/theoradec_hip.h, "While a frame is held").  Every named scenario asserts from the counter fe_pipelined that
it did reach that state before its ctl."""
import copy
import ctypes as C

import pytest

from oracle import ref
from tests import callscript as cs
from tests import refcmp, util
from tests.callscript import announce, empty, granpos, out, packet, pplevel, settle, stripe

pytestmark = pytest.mark.gpu
NAMES = list(cs.STREAMS)


def _counters(L):
    def read():
        v = []
        for name in (b"fe_pipelined", b"fe_pipeline_taken_back"):
            c = C.c_int()
            assert L.thip_get_option(name, C.byref(c)) == 0
            v.append(c.value)
        return tuple(v)
    return read


def _reference(s, script):
    refcmp.need_ref()
    rd = ref.RefDecoder(s["headers"])
    try:
        return cs.run(cs.RefSide(rd), script, s["packets"])
    finally:
        rd.close()


def _ours(hip, s, script, announcing=True, **opts):
    """(transcript, [(fe_pipelined, fe_pipeline_taken_back) before every operation and after the last])."""
    from theora_amd.decoder import Decoder
    L = hip._lib.load()
    with util.options(L, **opts):
        dec = Decoder(s["headers"])
        side = cs.OurSide(dec, announcing=announcing, counters=_counters(L))
        try:
            T = cs.run(side, script, s["packets"])
        finally:
            dec.close()
    return T, side.seen


def _held(seen, i_out):
    """Did the th_decode_ycbcr_out at operation i_out decode a frame ahead?"""
    return seen[i_out + 1][0] - seen[i_out][0] == 1


def _in_order(first, last):
    ops = []
    for i in range(first, last + 1):
        ops += [packet(i), out(1)]
    return ops


def _hold(s, key, extra=0):
    """(operations that end with packet c + 1 decoded ahead, c): packets 0 .. c in order, c + 1 (and `extra` more) announced, and
    the th_decode_ycbcr_out that takes it.  key: whether packet c + 1 is a key frame."""
    n = len(s["packets"])
    c = next(k - 1 for k in s["keys"] if k >= 3) if key else next(i - 1 for i in range(3, n) if i not in s["keys"] and i - 1 not in s["keys"])
    assert c + 6 < n
    return _in_order(0, c) + [announce(*range(c + 1, c + 3 + extra)), settle(), out(1)], c


def _scenario(hip, s, script, i_out, **opts):
    """Reference and ours (fe_pipeline on) over the script; a frame was held after operation i_out; the transcripts are equal."""
    want = _reference(s, script)
    got, seen = _ours(hip, s, script, fe_pipeline=1, **opts)
    assert _held(seen, i_out), "th_decode_ycbcr_out at operation %d did not decode a frame ahead:\n%s" % (i_out, cs.show(script, i_out))
    assert cs.compare(want, got, script) is None
    return want, got, seen


def _a_granpos(s):
    return (1234 << s["shift"]) + 1


@pytest.mark.parametrize("name", NAMES)
def test_post_processing_changes_the_streams_pictures(name):
    """The reference's own output at levels 0 and 7 differs: the pplevel scenarios below are not idle."""
    s = cs.stream(name)
    a = _reference(s, _in_order(0, 5))
    b = _reference(s, [pplevel(7)] + _in_order(0, 5))[1:]
    assert cs.compare(a, b, _in_order(0, 5), quiet=True) is not None


@pytest.mark.parametrize("name", NAMES)
def test_seek_with_a_frame_held(hip, name):
    """TH_DECCTL_SET_GRANPOS, then a key-frame packet from elsewhere: the granule positions count on from the value set."""
    s = cs.stream(name)
    pre, c = _hold(s, key=False)
    k = next(k for k in s["keys"] if k > c + 2)
    script = pre + [granpos(_a_granpos(s)), out(1), packet(k), out(1)] + _in_order(k + 1, min(k + 4, len(s["packets"]) - 1))
    _, got, seen = _scenario(hip, s, script, len(pre) - 1)
    assert seen[len(pre) + 1][1] - seen[len(pre)][1] == 1            # the ctl took the frame back


@pytest.mark.parametrize("key", [False, True], ids=["inter_held", "key_held"])
@pytest.mark.parametrize("name", NAMES)
def test_granpos_then_the_held_packet_itself(hip, name, key):
    s = cs.stream(name)
    pre, c = _hold(s, key=key)
    script = pre + [granpos(_a_granpos(s)), out(1)] + _in_order(c + 1, c + 5)
    _scenario(hip, s, script, len(pre) - 1)


@pytest.mark.parametrize("key", [False, True], ids=["inter_held", "key_held"])
@pytest.mark.parametrize("name", NAMES)
def test_granpos_then_a_dropped_frame_then_the_held_packet(hip, name, key):
    s = cs.stream(name)
    pre, c = _hold(s, key=key)
    script = pre + [granpos(_a_granpos(s)), out(1), empty(), out(1)] + _in_order(c + 1, c + 5)
    _scenario(hip, s, script, len(pre) - 1)


@pytest.mark.parametrize("name", NAMES)
def test_refused_requests_leave_the_held_frame_held(hip, name):
    """A negative granule position, a wrong buf_sz and level 8 return the reference's codes and change nothing: nothing is taken
    back, and the next th_decode_packetin still returns the frame decoded ahead."""
    s = cs.stream(name)
    pre, c = _hold(s, key=False)
    refused = [granpos(-5), granpos(_a_granpos(s), size=4), pplevel(8)]
    script = pre + refused + [out(1)] + _in_order(c + 1, c + 5)
    want, got, seen = _scenario(hip, s, script, len(pre) - 1)
    n = len(pre)
    assert [want[n + i]["rc"] for i in range(3)] == [cs.TH_EINVAL] * 3
    # (through the three refusals, the th_decode_ycbcr_out and the th_decode_packetin of the held packet)
    assert seen[n + 5][1] == seen[n][1], "a refused request took the frame back"
    assert seen[n + 5][0] == seen[n][0]


@pytest.mark.parametrize("level", [1, 2, 4, 7])
@pytest.mark.parametrize("key", [True, False], ids=["key_held", "inter_held"])
@pytest.mark.parametrize("name", NAMES)
def test_pplevel_with_a_frame_held(hip, name, key, level):
    """TH_DECCTL_SET_PPLEVEL while a frame is held: a held key frame is where the reference starts tracking (decode.c:1221-1227)
    and, from level 2, shows the filtered picture; a held inter frame it leaves unfiltered until the next key frame."""
    s = cs.stream(name)
    pre, c = _hold(s, key=key)
    script = pre + [pplevel(level), out(1)] + _in_order(c + 1, c + 5)
    want, _, _ = _scenario(hip, s, script, len(pre) - 1)
    if key and level >= 2:          # the filters did change the held frame's picture
        unfiltered = _reference(s, _in_order(0, c + 1))[-1]
        assert cs.compare([want[len(pre) + 3]], [unfiltered], [out(1)], quiet=True) is not None


@pytest.mark.parametrize("name", NAMES)
def test_the_pipeline_stands_down_for_post_processing_and_comes_back(hip, name):
    """Level 7, three frames, level 0, packets announced all along: no frame goes ahead while post-processing is on, and the
    first th_decode_ycbcr_out after level 0 takes one again."""
    s = cs.stream(name)
    script = [packet(0), out(1), announce(1, 2), settle(), out(1)]
    i_hold = len(script) - 1
    script += [pplevel(7), packet(1), announce(2, 3), settle(), out(1)]            # (taken back; packet 1 drops what was announced)
    script += [packet(2), announce(4), settle(), out(1), packet(3), announce(5), settle(), out(1)]
    i_pp_end = len(script)
    script += [pplevel(0), packet(4), out(1)]
    i_back = len(script) - 1
    script += _in_order(5, 8)
    _, _, seen = _scenario(hip, s, script, i_hold)
    assert seen[i_pp_end][0] == seen[i_hold + 1][0], "a frame went ahead while post-processing was on"
    assert _held(seen, i_back), "the pipeline did not come back after level 0"


@pytest.mark.parametrize("name", NAMES)
def test_stripe_callback_set_with_a_frame_held(hip, name):
    """The callback is made for the held frame (inside its th_decode_packetin), its ranges cover the frame and the picture they
    declare ready is the reference's; switched off, it is not made any more."""
    s = cs.stream(name)
    pre, c = _hold(s, key=False)
    script = pre + [stripe(True), out(1), packet(c + 1), out(1), packet(c + 2), stripe(False), packet(c + 3), out(1)]
    want, got, _ = _scenario(hip, s, script, len(pre) - 1)
    n = len(pre)
    rows = list(range(-(-s["h"] // 8)))
    for T in (want, got):
        for k in (n + 2, n + 4):
            assert cs.rows_covered(T[k]["stripes"]) == rows, T[k]["stripes"]
        assert T[n + 6]["stripes"] == []
        assert refcmp.diff_planes(T[n + 2]["stripe_picture"], T[n + 3]["pictures"][0]) == []


@pytest.mark.parametrize("name", NAMES)
def test_pictures_asked_for_twice_and_not_at_all(hip, name):
    s = cs.stream(name)
    pre, c = _hold(s, key=False)
    script = pre + [out(2), packet(c + 1), out(0), packet(c + 2), out(2), empty(), out(2)] + _in_order(c + 3, c + 5)
    _scenario(hip, s, script, len(pre) - 1)


@pytest.mark.parametrize("name", NAMES)
def test_free_with_a_frame_held_and_packets_announced(hip, name):
    """th_decode_free with a frame held and two announcements outstanding; a fresh context on the same stream then decodes its
    first four frames like the reference."""
    s = cs.stream(name)
    pre, c = _hold(s, key=False, extra=1)              # c + 1 held, c + 2 and c + 3 announced
    want = _reference(s, pre)
    got, seen = _ours(hip, s, pre, fe_pipeline=1)       # (closes the context with the frame held)
    assert _held(seen, len(pre) - 1)
    assert cs.compare(want, got, pre) is None
    script = _in_order(0, 3)
    got, _ = _ours(hip, s, script, fe_pipeline=1)
    assert cs.compare(_reference(s, script), got, script) is None


CONFIGS = {   # name: (announcements made, library options)
    "never_announced": (False, dict(fe_pipeline=1)),
    "pipelined": (True, dict(fe_pipeline=1)),
    "announced_not_pipelined": (True, dict(fe_pipeline=0)),
}
_WANT = {}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("seed", cs.SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_random_scripts_equal_the_reference(hip, name, seed, config):
    s = cs.stream(name)
    script, forced = cs.gpu_script(name, seed)
    if (name, seed) not in _WANT:                       # (the reference's transcript once for the three configurations, never changed)
        _WANT[name, seed] = _reference(s, script)
    announcing, opts = CONFIGS[config]
    got, seen = _ours(hip, s, script, announcing=announcing, **opts)
    assert cs.compare(_WANT[name, seed], got, script, seed=(name, seed, config)) is None
    ahead, back = seen[-1][0] - seen[0][0], seen[-1][1] - seen[0][1]
    print(name, seed, config, "operations", len(script), "fe_pipelined", ahead, "fe_pipeline_taken_back", back)
    if config == "pipelined":
        for i_out, i_ctl, kind, follower in forced:
            assert _held(seen, i_out), (kind, follower, "no frame was held at operation %d" % i_out, cs.show(script, i_ctl))
        assert ahead >= len(forced) and back >= 1
    else:
        assert ahead == 0 and back == 0


def test_the_comparison_notices_one_altered_value(hip):
    """One granule position and one pixel of a transcript of ours changed: compare() names each operation."""
    s = cs.stream("420")
    script, _ = cs.gpu_script("420", 0)
    want = _reference(s, script)
    got, _ = _ours(hip, s, script, fe_pipeline=1)
    assert cs.compare(want, got, script) is None
    k_pkt = [k for k, e in enumerate(got) if e and "granpos" in e and e["rc"] == 0][-1]
    k_out = [k for k, e in enumerate(got) if e and e.get("pictures")][-1]
    alt = copy.deepcopy(got)
    alt[k_pkt]["granpos"] += 1
    assert cs.compare(want, alt, script, seed=5, quiet=True)[:2] == (5, k_pkt)
    alt = copy.deepcopy(got)
    alt[k_out]["pictures"][-1][1][2, 3] ^= 1
    d = cs.compare(want, alt, script, seed=6, quiet=True)
    assert d[:2] == (6, k_out) and "1 pixels differ" in d[2]
