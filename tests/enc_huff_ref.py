"""enc_huff_ref.py -- TEST INFRASTRUCTURE: a restatement of include/theoraenc_hip.h's "Huffman codes": the check of a code set, the
setup header's trees from the codes, the packet's token histogram and the trainer thip_huff_train, to compare the library with bit
for bit; and two families of legal code sets that are nothing like the built-in ones.

A code set is an (80, 32, 2) integer array of (pattern, nbits), as theora_amd.encoder takes and returns it."""
import numpy as np

from tests.streamgen import eob_token

M64 = (1 << 64) - 1


# ---- code sets ------------------------------------------------------------------------------------------------------------------
def set_valid(cs):
    """One set of 32 (pattern, nbits): every token has a code of 1..32 bits, and the codes' intervals of 32-bit strings tile
    [0, 2^32): full and prefix-free.  -> the tokens by rising code, or None."""
    iv = []
    for tok in range(32):
        pat, nb = int(cs[tok][0]), int(cs[tok][1])
        if nb < 1 or nb > 32:
            return None
        iv.append(((pat & ((1 << nb) - 1)) << (32 - nb), tok, nb))
    iv.sort()
    at = 0
    for start, _, nb in iv:
        if start != at:
            return None
        at += 1 << (32 - nb)
    return [tok for _, tok, _ in iv] if at == 1 << 32 else None


def valid(codes):
    return all(set_valid(codes[h]) is not None for h in range(80))


def masked(codes):
    c = np.array(codes, np.int64)
    c[..., 0] &= (np.int64(1) << c[..., 1]) - 1
    return c


def tree_bits(codes):
    """The 80 trees as the setup header states them (spec 6.4.4), a string of '0' and '1': pre-order, the 0 branch first."""
    out = []
    for h in range(80):
        strings = {format(int(p) & ((1 << int(n)) - 1), "0%db" % int(n)): tok for tok, (p, n) in enumerate(codes[h])}

        def rec(prefix):
            if prefix in strings:
                out.append("1" + format(strings[prefix], "05b"))
            else:
                assert len(prefix) < 32
                out.append("0")
                rec(prefix + "0")
                rec(prefix + "1")
        rec("")
    return "".join(out)


def codes_of_setup(setup):
    """tests.enc_ref.SetupParams -> the code set its trees state."""
    return np.array([[(int(setup.codes[h][tok], 2), len(setup.codes[h][tok])) for tok in range(32)] for h in range(80)], np.int64)


def canonical(lengths):
    """A full prefix code with these lengths (Kraft sum 1): the shorter code first, ties to the lower token."""
    order = sorted(range(32), key=lambda t: (lengths[t], t))
    out, code, prev = [None] * 32, 0, lengths[order[0]]
    for t in order:
        code <<= lengths[t] - prev
        prev = lengths[t]
        out[t] = (code, lengths[t])
        code += 1
    assert code == 1 << prev
    return out


def comb_codes(order=lambda h: list(range(32))):
    """Lengths 1, 2, ..., 30, 31, 31: the deepest full code of 32 leaves.  order(h): set h's tokens from the shortest code to the
    longest."""
    codes = np.zeros((80, 32, 2), np.int64)
    for h in range(80):
        toks = list(order(h))
        assert sorted(toks) == list(range(32))
        for k, tok in enumerate(toks):
            codes[h, tok] = ((1 << (k + 1)) - 2, k + 1) if k < 31 else ((1 << 31) - 1, 31)
    return codes


def comb_order(h, last=None):
    """A token order that differs from set to set; last: the token that gets a 31-bit code."""
    toks = [(7 * k + 3 * h + 5) % 32 for k in range(32)]
    if last is not None:
        toks.remove(last)
        toks.append(last)
    return toks


def rotated_codes(builtin, shift=11):
    """The built-in lengths of each set moved between tokens (token t takes the length of token (t + shift + set) % 32)."""
    codes = np.zeros((80, 32, 2), np.int64)
    for h in range(80):
        lengths = [int(builtin[h][(t + shift + h) % 32][1]) for t in range(32)]
        codes[h] = canonical(lengths)
    return codes


# ---- the packet's histogram -----------------------------------------------------------------------------------------------------------
def huff_group(z):
    return 0 if z == 0 else 1 if z <= 5 else 2 if z <= 14 else 3 if z <= 27 else 4


def hist_of_words(words):
    """The merged tokens' histogram [5][2][32] from the tokens before the merge in stream order (the word format of thip_encode.h:
    token | extra << 5 | index << 16 | plane << 22; an EOB has token and extra 0): maximal runs of EOBs in pieces of at most 4095,
    each counted in the list of its first EOB."""
    hist = np.zeros((5, 2, 32), np.int64)
    run, first = 0, None

    def flush():
        nonlocal run
        if run:
            hist[huff_group((first >> 16) & 63), int((first >> 22) != 0), eob_token(run)[0]] += 1
            run = 0
    for w in (int(x) for x in words):
        if (w & 0xFFFF) == 0:
            if not run:
                first = w
            run += 1
            if run == 4095:
                flush()
            continue
        flush()
        hist[huff_group((w >> 16) & 63), int((w >> 22) != 0), w & 31] += 1
    flush()
    return hist


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def huffman(weights):
    """The Huffman code of 32 integer weights by the rule of the built-in trees -> [(pattern, nbits)]."""
    nodes = [(int(w) & M64, None, None) for w in weights]
    live = list(range(32))
    while len(live) > 1:
        a = min(live, key=lambda x: (nodes[x][0], x))
        b = min((x for x in live if x != a), key=lambda x: (nodes[x][0], x))
        nodes.append(((nodes[a][0] + nodes[b][0]) & M64, a, b))
        live = [x for x in live if x not in (a, b)] + [len(nodes) - 1]
    out = [None] * 32

    def walk(x, code, n):
        if nodes[x][1] is None:
            out[x] = (code, n)
            return
        walk(nodes[x][1], code << 1, n + 1)
        walk(nodes[x][2], code << 1 | 1, n + 1)
    walk(live[0], 0, 0)
    return out


def _assign(samples, lens):
    """samples: (kind, counts) with counts [1 or 4][32] uint64; lens [80][32] uint64 -> (tables, total cost mod 2^64)."""
    tables, total = [], 0
    for ac, cnt in samples:
        groups = range(1, 5) if ac else range(0, 1)
        cost = [sum(int((cnt[k] * lens[16 * hg + t]).sum(dtype=np.uint64)) for k, hg in enumerate(groups)) & M64 for t in range(16)]
        t = min(range(16), key=lambda t: (cost[t], t))
        tables.append(t)
        total = (total + cost[t]) & M64
    return tables, total


def train(hists, start, rounds=8):
    """thip_huff_train, restated -> (codes, stats).  hists: (5, 2, 32) count arrays; start: a code set."""
    assert valid(start) and 1 <= rounds <= 64 and len(hists) <= 1 << 20
    samples = []
    for h in hists:
        h = np.asarray(h).astype(np.uint64)
        for cls in range(2):
            for ac in range(2):
                cnt = h[1:5, cls] if ac else h[0:1, cls]
                if cnt.any():
                    samples.append((ac, cnt))
    cur = masked(start)
    assign, B = _assign(samples, cur[..., 1].astype(np.uint64))
    B0, accepted = B, 0
    for _ in range(rounds):
        nxt = cur.copy()
        for ac in range(2):
            for t in range(16):
                mine = [cnt for (a, cnt), tt in zip(samples, assign) if a == ac and tt == t]
                if not mine:
                    continue
                for k, hg in enumerate(range(1, 5) if ac else range(0, 1)):
                    H = [sum(int(cnt[k][tok]) for cnt in mine) & M64 for tok in range(32)]
                    nxt[16 * hg + t] = huffman([(1024 * x + 1) & M64 for x in H])
        trial, B1 = _assign(samples, nxt[..., 1].astype(np.uint64))
        if B1 >= B:
            break
        cur, assign, B, accepted = nxt, trial, B1, accepted + 1
    used = [len({t for (a, _), t in zip(samples, assign) if a == ac}) for ac in range(2)]
    return cur, dict(bits_start=B0, bits_end=B, rounds=accepted, dc_tables=used[0], ac_tables=used[1], samples=len(samples))


def token_cost(hist, codes, huff):
    """The code bits of a packet with this histogram under the tables huff (DC luma, DC chroma, AC luma, AC chroma)."""
    return sum(int(hist[hg, ch] @ codes[16 * hg + huff[(2 if hg else 0) + ch], :, 1]) for hg in range(5) for ch in range(2))
