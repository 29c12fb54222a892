"""packref.py -- TEST INFRASTRUCTURE: the plain reference of th_encode_*'s device packetiser (theora_amd/csrc/thip_encode_pack.h,
driven through thip_enc_pack_tokens), and builders of the token streams that reach its span, run and bit edges.

pack() is a direct loop over the stream in the manner of enc_ref.encode_frame's last third, to which tests/test_packref_cpu.py pins
it; unpack() reads the bits back the way a decoder does, so unpack(pack(x)) == x checks the reference against itself.  Nothing here
knows of spans, tiles or work groups.

A token word is token | extra bits << 5 | zig-zag index << 16 | plane << 22 (thip_encode.h); token 0 is a block's EOB, the others
are 7..31.  list_len is [64][3]: the tokens of (index, plane), the stream being ordered by index, then plane."""
import numpy as np

EXTRA_BITS = (0, 0, 0, 2, 3, 4, 12, 3, 6, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4, 5, 6, 10, 1, 1, 1, 1, 1, 3, 4, 2, 3)   # spec Table 7.38
RUN_CAP = 4095
VALUE_TOKENS = tuple(range(7, 32))
LUMA_TOKENS, CHROMA_TOKENS = tuple(range(7, 32, 2)), tuple(range(8, 32, 2))   # disjoint alphabets for tables("pick") / ("ties")


def huff_group(z):
    return 0 if z == 0 else 1 if z <= 5 else 2 if z <= 14 else 3 if z <= 27 else 4


def eob_token(run):
    """(token, extra) of a run of 1..4095 EOBs."""
    assert 1 <= run <= RUN_CAP
    if run <= 3:
        return run - 1, 0
    if run <= 7:
        return 3, run - 4
    if run <= 15:
        return 4, run - 8
    if run <= 31:
        return 5, run - 16
    return 6, run


def eob_run(tok, extra):
    return tok + 1 if tok <= 2 else 4 + extra if tok == 3 else 8 + extra if tok == 4 else 16 + extra if tok == 5 else extra


def word(tok, extra, z, p):
    return tok | extra << 5 | z << 16 | p << 22


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def merge(words, list_len):
    """The merged tokens in stream order: [(index, plane, token, extra)].  Runs of EOBs merge across lists and planes; a run is cut
    into pieces of 4095 from its start, and a piece belongs to the list of its first EOB."""
    words = [int(w) for w in words]
    assert int(np.sum(list_len)) == len(words)
    merged, run, rz, rp, at = [], 0, 0, 0, 0

    def flush():
        nonlocal run
        if run:
            merged.append((rz, rp) + eob_token(run))
            run = 0
    for z in range(64):
        for p in range(3):
            for _ in range(int(list_len[z][p])):
                w = words[at]
                at += 1
                assert (w >> 16 & 63, w >> 22) == (z, p), (at - 1, hex(w), z, p)   # the words carry their own list
                tok = w & 31
                if tok == 0:
                    if run == 0:
                        rz, rp = z, p
                    run += 1
                    if run == RUN_CAP:
                        flush()
                    continue
                assert tok >= 7, hex(w)
                flush()
                merged.append((z, p, tok, w >> 5 & 0x7FF))
    flush()
    return merged


def choose_tables(merged, lens):
    """[DC luma, DC chroma, AC luma, AC chroma]: for each the table, of its 16, that codes its tokens in the fewest bits (code
    lengths alone: the extra bits are the same in every table); a tie goes to the lower index.  DC is Huffman group 0, AC groups
    1..4 with one index for all four."""
    hist = np.zeros((5, 2, 32), np.int64)
    for z, p, tok, _ in merged:
        hist[huff_group(z), int(p > 0), tok] += 1
    lens = np.asarray(lens, np.int64)
    hti = []
    for c in range(4):
        ac, ch = c >> 1, c & 1
        best, best_t = None, 0
        for t in range(16):
            cost = sum(int(hist[hg, ch] @ lens[16 * hg + t]) for hg in (range(1, 5) if ac else range(1)))
            if best is None or cost < best:
                best, best_t = cost, t
        hti.append(best_t)
    return hti


def pack(words, list_len, codes, lens, phase):
    """(the packet's bytes from byte 0, the record).  Bits are MSB first from bit `phase` of byte 0, the bits before them zero: the
    DC table indices, the tokens in stream order, and the AC table indices where index 1 begins -- in front of the first merged
    token of an index above 0, at the end when there is none."""
    assert 0 <= phase <= 7
    merged = merge(words, list_len)
    hti = choose_tables(merged, lens)
    acc, n = 0, phase   # the bits so far as one integer

    def put(v, nb):
        nonlocal acc, n
        assert 0 <= v < 1 << nb
        acc = acc << nb | v
        n += nb
    put(hti[0] << 4 | hti[1], 8)
    ac_done, bits = False, 0
    for z, p, tok, extra in merged:
        if z > 0 and not ac_done:
            put(hti[2] << 4 | hti[3], 8)
            ac_done = True
        h = 16 * huff_group(z) + hti[(2 if z else 0) + int(p > 0)]
        put(int(codes[h][tok]), int(lens[h][tok]))
        put(extra, EXTRA_BITS[tok])
        bits += int(lens[h][tok]) + EXTRA_BITS[tok]
    if not ac_done:
        put(hti[2] << 4 | hti[3], 8)
    assert n == phase + 16 + bits
    nbytes = (n + 7) >> 3
    data = (acc << (8 * nbytes - n)).to_bytes(nbytes, "big")
    rec = dict(bits=bits, bytes=nbytes, tokens=len(words), merged=len(merged), merged_ac=sum(m[0] > 0 for m in merged), huff=hti)
    return data, rec


def unpack(data, phase, codes, lens, list_len):
    """What a decoder makes of pack()'s bytes, given prefix-free tables and the lengths of the lists before the merge: (the words,
    EOB runs expanded again; the four table indices; the bits read, `phase` included).  The AC indices are read where a decoder
    reads them: when index 1 begins, whatever run is still open."""
    bits = "".join(format(b, "08b") for b in data)
    pos = phase
    assert set(bits[:phase]) <= {"0"}

    def read(nb):
        nonlocal pos
        assert pos + nb <= len(bits)
        v = int(bits[pos:pos + nb], 2) if nb else 0
        pos += nb
        return v
    decode = {}

    def token(h):
        if h not in decode:
            decode[h] = {(int(lens[h][t]), int(codes[h][t])): t for t in range(32)}
            assert len(decode[h]) == 32
        for nb in range(1, 33):
            t = decode[h].get((nb, int(bits[pos:pos + nb], 2)))
            if t is not None:
                read(nb)
                return t
        raise AssertionError("no code at bit %d" % pos)
    hti = [read(4), read(4), None, None]
    words, carry = [], 0
    for z in range(64):
        if z == 1:
            hti[2:] = [read(4), read(4)]
        for p in range(3):
            left = int(list_len[z][p])
            while left:
                if carry:
                    k = min(carry, left)
                    words += [word(0, 0, z, p)] * k
                    carry -= k
                    left -= k
                    continue
                tok = token(16 * huff_group(z) + hti[(2 if z else 0) + int(p > 0)])
                extra = read(EXTRA_BITS[tok])
                if tok <= 6:
                    carry = eob_run(tok, extra)
                    assert 1 <= carry <= RUN_CAP
                else:
                    words.append(word(tok, extra, z, p))
                    left -= 1
    assert carry == 0
    assert set(bits[pos:]) <= {"0"} and len(bits) - pos < 8
    return np.array(words, np.uint32), hti, pos


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def lists_from(spec):
    """list_len from {(index, plane): tokens}."""
    ll = np.zeros((64, 3), np.int64)
    for (z, p), n in spec.items():
        ll[z][p] = n
    return ll


def lists(T, first_ac, rng):
    """A list_len of T tokens whose first token of an index above 0 is at stream index first_ac (None, or T: there is none; 0: the
    index-0 lists are empty).  The index-0 tokens are split over the three planes, the others over a handful of later lists."""
    first_ac = T if first_ac is None else first_ac
    assert 0 <= first_ac <= T
    ll = np.zeros((64, 3), np.int64)
    ll[0] = rng.multinomial(first_ac, [0.5, 0.25, 0.25])
    rest = T - first_ac
    if rest:
        zs = np.sort(rng.choice(np.arange(1, 64), size=min(6, rest), replace=False))
        share = rng.multinomial(rest - len(zs), np.ones(len(zs) * 3) / (len(zs) * 3)).reshape(len(zs), 3)
        share[:, 0] += 1   # (every chosen index has a token, the first of them at first_ac)
        ll[zs] = share
    assert ll.sum() == T and ll[0].sum() == first_ac
    return ll


def stream_lists(list_len):
    """(index, plane) of every stream position."""
    n = np.asarray(list_len, np.int64).reshape(-1)
    return np.stack([np.repeat(np.arange(192) // 3, n), np.repeat(np.arange(192) % 3, n)], axis=1)


def stream(list_len, eob_mask, rng, tokens=None):
    """The words of a stream: an EOB where eob_mask says so, elsewhere a value or zero-run token with random extra bits -- any of
    7..31, or of tokens = (luma's alphabet, chroma's alphabet).  The (index, plane) fields follow list_len's order."""
    zp = stream_lists(list_len)
    eob_mask = np.asarray(eob_mask, bool)
    assert eob_mask.shape == (len(zp),)
    tok = np.zeros(len(zp), np.int64)
    for ch in range(2):
        sel = ~eob_mask & ((zp[:, 1] > 0) == bool(ch))
        tok[sel] = rng.choice(VALUE_TOKENS if tokens is None else tokens[ch], size=int(sel.sum()))
    extra = rng.integers(0, 1 << np.asarray(EXTRA_BITS)[tok])   # (an EOB has none)
    return (tok | extra << 5 | zp[:, 0] << 16 | zp[:, 1] << 22).astype(np.uint32)


def mask(T, density, rng):
    """EOBs at random with the given density."""
    return rng.random(T) < density


def run_mask(T, start, length, rng, density=0.3):
    """A random mask in which [start, start + length) is one whole run: EOBs throughout, no EOB next to it."""
    assert 0 <= start and length >= 1 and start + length <= T
    m = mask(T, density, rng)
    m[start:start + length] = True
    if start:
        m[start - 1] = False
    if start + length < T:
        m[start + length] = False
    return m


_default = None


def default_tables():
    """The encoder's own 80 tables, read back from its setup header."""
    global _default
    if _default is None:
        from tests import enc_ref
        from theora_amd.encoder import Encoder
        e = Encoder(64, 48, 0, 32)
        setup = enc_ref.SetupParams(e.header_packets()[2])
        e.close()
        codes, lens = np.zeros((80, 32), np.uint32), np.zeros((80, 32), np.uint8)
        for h in range(80):
            for t in range(32):
                codes[h][t], lens[h][t] = int(setup.codes[h][t], 2), len(setup.codes[h][t])
        _default = (codes, lens)
    return _default[0].copy(), _default[1].copy()


def _random_codes(lens, rng):
    return (rng.integers(0, 1 << 32, lens.shape, dtype=np.uint64) >> (32 - lens.astype(np.uint64))).astype(np.uint32)


def tables(kind, rng=None, want=None):
    """(codes [80][32] uint32, lens [80][32] uint8).  Only "default" is prefix-free: the kernels never decode, and random codes make
    a token coded with the wrong table show in the bytes.
      default   the encoder's own
      len32     every length 32 (with the 10 extra bits of token 22: 42 bits a token, the most a tile can be made to hold)
      len1      every length 1
      pick      want = four tuples of table indices (DC luma, DC chroma, AC luma, AC chroma): for a stream whose luma tokens come
                from LUMA_TOKENS and chroma tokens from CHROMA_TOKENS, the tables of want[c] are the cheapest of class c, EXACTLY
                tied among themselves, whatever the histogram (as long as the class has a token of its alphabet): they cost 2..6
                bits a token where every other table costs 12..20, and the EOB-run tokens cost the same in all 16 tables of a group
      ties      pick with two tied tables in every class"""
    if kind == "default":
        return default_tables()
    if kind in ("len32", "len1"):
        lens = np.full((80, 32), 32 if kind == "len32" else 1, np.uint8)
        return _random_codes(lens, rng), lens
    if kind == "ties":
        kind, want = "pick", [tuple(sorted(int(t) for t in rng.choice(16, 2, replace=False))) for _ in range(4)]
    assert kind == "pick" and len(want) == 4
    lens = rng.integers(12, 21, (80, 32)).astype(np.uint8)
    for hg in range(5):
        lens[16 * hg:16 * hg + 16, :7] = lens[16 * hg, :7]
        for ch, alphabet in enumerate((LUMA_TOKENS, CHROMA_TOKENS)):
            cheap = rng.integers(2, 7, len(alphabet))
            for t in want[(2 if hg else 0) + ch]:
                lens[16 * hg + t, list(alphabet)] = cheap
    return _random_codes(lens, rng), lens
