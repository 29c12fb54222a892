"""tests/callscript.py without a device: the generated call scripts through the reference decoder and through th_decode_* in
slot-trace mode (refcmp.trace_mode(): th_decode_packetin, TH_DECCTL_SET_GRANPOS and the empty-packet path run, the slot calls
are recorded and the oracle makes the pictures from them).  Pins the generator, the runner and the reference side where there is
no GPU, and keeps the plain path's granule arithmetic under test.  Slot-trace mode has neither post-processing nor a stripe
callback, so the scripts are drawn without them, and announcements are left out."""
import copy

import numpy as np
import pytest

import oracle
from oracle import ref
from tests import callscript as cs
from tests import refcmp


class TracedSide:
    """theora_amd.decoder.Decoder in slot-trace mode, its slot calls fed to the oracle."""
    ours = False            # (announcements and settling are left out)

    def __init__(self, dec, s):
        self.dec, self.ost, self.started = dec, oracle.State(s["w"], s["h"], s["fmt"]), False
        hd, vd = int(not (s["fmt"] & 1)), int(not (s["fmt"] & 2))
        self.grey = [np.full((s["h"], s["w"]), 0x80, np.uint8)] + [np.full((s["h"] >> vd, s["w"] >> hd), 0x80, np.uint8)] * 2

    def packetin(self, data):
        rc, gp = self.dec.packetin_raw(data)
        if rc == 0:
            assert refcmp.oracle_apply_trace(self.ost, self.dec.slot_trace()) == 0
            self.started = True
        return rc, gp

    def out(self):
        # (before the first frame the reference shows its mid-grey dummy once a dropped frame has made it, decode.c:2757-2762)
        return [p.copy() for p in (refcmp.oracle_picture(self.ost) if self.started else self.grey)]

    def ctl(self, req, obj, size):
        return self.dec.ctl(req, obj, size)

    def before(self, k):
        pass

    def close(self):
        self.dec.close()
        self.ost.close()


def _reference(s, script):
    rd = ref.RefDecoder(s["headers"])
    try:
        return cs.run(cs.RefSide(rd), script, s["packets"])
    finally:
        rd.close()


@pytest.mark.parametrize("seed", cs.SEEDS)
@pytest.mark.parametrize("name", list(cs.STREAMS))
def test_generated_scripts_in_slot_trace_mode_equal_the_reference(name, seed):
    from theora_amd.decoder import Decoder
    refcmp.need_ref()
    s = cs.stream(name)
    script, forced = cs.generate(7000 + seed, len(s["packets"]), s["keys"], nops=40, ctls=False, shift=s["shift"])
    assert [f[2] for f in forced] == ["granpos_legal", "granpos_refused"]
    assert not any(op[0] in ("pplevel", "stripe") for op in script)
    want = _reference(s, script)
    with refcmp.trace_mode():
        side = TracedSide(Decoder(s["headers"]), s)
        try:
            got = cs.run(side, script, s["packets"])
        finally:
            side.close()
    assert cs.compare(want, got, script, seed=(name, seed)) is None
    assert sum(1 for e in want if e and e.get("rc") == cs.TH_EINVAL) >= 1        # the refusal went through both


def test_every_gpu_script_runs_through_the_reference_as_intended():
    """Every script tests/test_gpu_call_scripts.py draws, through the reference alone: no call fails that the script did not draw
    as a refusal (TH_EINVAL, TH_EFAULT or TH_EBADPACKET, from a ctl drawn as refused), every forced pattern is there, every
    operation is used somewhere, and pictures come out."""
    refcmp.need_ref()
    used, pairs, filtered = set(), set(), 0
    for name in cs.STREAMS:
        s = cs.stream(name)
        for seed in cs.SEEDS:
            script, forced = cs.gpu_script(name, seed)
            assert 40 <= len(script) <= 64, len(script)
            assert [f[2] for f in forced] == list(cs.FORCED_CTLS)
            pairs |= {(f[2], f[3]) for f in forced}
            for i_out, i_ctl, kind, follower in forced:
                assert script[i_out] == cs.out(1) and i_ctl == i_out + 1 and script[i_out - 1] == cs.settle()
                c = script[i_out - 3][1]
                assert script[i_out - 3][0] == "packet" and script[i_out - 2] == cs.announce(c + 1, c + 2)
                if kind == "pplevel_key":
                    assert c + 1 in s["keys"] and script[i_ctl][0] == "pplevel" and script[i_ctl][1] >= 2
                if kind == "granpos_refused":
                    assert cs.intended_refusal(script[i_ctl]) == cs.TH_EINVAL
                nxt = script[i_ctl + 1]
                assert nxt == {"announced": cs.packet(c + 1), "empty_then_announced": cs.empty()}.get(follower, nxt)
                if follower == "other_key":
                    assert nxt[0] == "packet" and nxt[1] in s["keys"] and nxt[1] != c + 1
            T = _reference(s, script)
            for k, (op, e) in enumerate(zip(script, T)):
                used.add(op[0])
                if e is None or "pictures" in e:
                    continue
                want = cs.intended_refusal(op)
                if want is not None:
                    assert want in (cs.TH_EINVAL, cs.TH_EFAULT, cs.TH_EBADPACKET) and e["rc"] == want, (name, seed, k, op, e["rc"])
                else:
                    assert e["rc"] >= 0, (name, seed, k, op, e["rc"], cs.show(script, k))
                if op[0] == "ppmax":
                    assert e["value"] == 7
            plain = _reference(s, [op for op in script if op[0] not in ("pplevel", "stripe")])
            filtered += int(cs.compare(T, _with_gaps(script, plain), script, quiet=True) is not None)
    assert used == {"packet", "empty", "out", "granpos", "pplevel", "stripe", "ppmax", "announce", "settle"}
    assert len(pairs) == len(cs.FORCED_CTLS) * len(cs.FORCED_FOLLOWERS)
    assert filtered >= len(cs.STREAMS) * len(cs.SEEDS) // 2         # post-processing and stripes are not idle in the scripts


def _with_gaps(script, plain):
    """The transcript of the script without its pplevel and stripe operations, with entries for them put back (a ctl that went
    well), so that the two can be compared."""
    it, outp = iter(plain), []
    for op in script:
        if op[0] in ("pplevel", "stripe"):
            outp.append(dict(rc=cs.intended_refusal(op) or 0, value=None))
        else:
            outp.append(next(it))
    return outp


def test_the_comparison_notices_one_altered_value_without_a_device():
    refcmp.need_ref()
    s = cs.stream("444")
    script, _ = cs.generate(7001, len(s["packets"]), s["keys"], nops=40, ctls=False, shift=s["shift"])
    T = _reference(s, script)
    assert cs.compare(T, copy.deepcopy(T), script) is None
    k_pkt = next(k for k, e in enumerate(T) if e and "granpos" in e and k > 10)
    k_out = next(k for k, e in enumerate(T) if e and e.get("pictures") and k > 10)
    alt = copy.deepcopy(T)
    alt[k_pkt]["granpos"] += 1
    assert cs.compare(T, alt, script, seed=1, quiet=True)[:2] == (1, k_pkt)
    alt = copy.deepcopy(T)
    alt[k_out]["pictures"][0][2][3, 5] ^= 1
    assert cs.compare(T, alt, script, seed=2, quiet=True)[:2] == (2, k_out)
