"""Hand-made packed documents for the record route of the edge-feature producer (test_producer_rec_cpu.py, test_producer_rec_gpu.py)
and a numpy restatement of what gcgcn_tensorise writes from their slot records.  Importable without a GPU.

A slot record is (u, v, j, s0, s1, h0, h1, t0, t1): entity pair, sentence slot, sentence token range, head and tail mention range.
BATCHES["hand"] gives (B, N, S, T) = (3, 5, 3, 70) and covers: a live slot and slots whose range misses token 0; s0 < 0 and s1 > T;
ranges that cross t = 64; a pair with slots 0 and 2 live and slot 1 dead; a pair whose only live slot is slot 1; records with j >= S;
empty and inverted ranges; mentions left of, inside and right of the sentence; distances >= 512 on either side; a one-token range; a
document with no records at all; a document with n_valid < N, one of whose live records names an entity at or past its n_valid
(u < N: the bit is set, the scan masks it, no row may be stored for it).  No pair of "hand" has all S slots live; BATCHES["t1"],
(2, 3, 2, 1), has one (divided by 1e-10, glove:205).  BATCHES["none_live"] is a batch whose ranges all miss token 0."""
import numpy as np

from gcgcn_amd.data import PackedDoc

I32 = np.int32


def doc(n, n_tokens, slots, max_sentence_num, seed=0, n_rel=4):
    """A PackedDoc with n entities (one mention each), n_tokens tokens and the given slot records."""
    r = np.random.default_rng(seed)
    tokens = r.integers(1, 20, (n_tokens, 3)).astype(I32)
    tokens[:, 2] = r.integers(0, 7, n_tokens)
    starts = r.integers(0, max(n_tokens - 1, 1), n)
    mentions = np.stack([starts, np.minimum(starts + 1 + r.integers(0, 2, n), n_tokens)], 1).astype(I32)
    mentions[:, 1] = np.maximum(mentions[:, 1], mentions[:, 0] + 1)
    slots = np.asarray(slots, I32).reshape(-1, 9)
    pairs = sorted({(int(u), int(v)) for u, v in slots[:, :2]})
    labels = [(u, v, (u + v) % n_rel) for u, v in pairs[:3]]
    return PackedDoc(tokens, r.integers(1, 7, n).astype(I32), np.arange(n + 1, dtype=I32), mentions, slots,
                     np.asarray(pairs, I32).reshape(-1, 2), np.asarray(labels, I32).reshape(-1, 3), n_rel, max_sentence_num)


def hand(n_rel=4):
    d0 = doc(5, 70, [
        (0, 1, 0, 0, 20, 3, 5, 10, 12),            # live; both mentions inside the sentence
        (0, 1, 1, 25, 40, 26, 28, 30, 31),         # dead: misses token 0
        (0, 1, 2, -5, 30, 40, 45, 2, 4),           # live, s0 < 0; head mention right of the sentence
        (0, 2, 0, 0, 90, 600, 610, -700, -690),    # live, s1 > T, crosses t = 64; distances >= 512 to the right and to the left
        (0, 2, 1, 0, 66, -8, -6, 50, 52),          # live, crosses t = 64; head mention left of the sentence
        (1, 0, 0, 0, 1, 0, 1, 5, 6),               # live, one token
        (2, 3, 1, 0, 8, 1, 3, 4, 7),               # the pair's only live slot is slot 1
        (3, 4, 0, 5, 5, 1, 2, 3, 4),               # empty range
        (3, 4, 1, 10, 5, 1, 2, 3, 4),              # inverted range
        (3, 4, 2, 0, 0, 1, 2, 3, 4),               # empty at token 0
        (4, 4, 2, 0, 33, 10, 13, 10, 13),          # live, the diagonal
        (1, 2, 3, 0, 10, 1, 2, 3, 4),              # j >= S: dropped
        (1, 2, 5, 0, 10, 1, 2, 3, 4),              # j >= S: dropped
        (3, 1, 0, 30, 50, 31, 33, 40, 44),         # dead, in the middle
        (4, 0, 1, 63, 70, 64, 65, 66, 67),         # dead, at the end
        (2, 1, 0, -3, 65, 520, 530, 0, 2),         # live, s0 < 0, crosses t = 64, head distance >= 512
    ], 3, seed=1, n_rel=n_rel)
    d1 = doc(5, 41, [], 1, seed=2, n_rel=n_rel)                 # no records at all
    d2 = doc(3, 55, [                              # n_valid = 3 < N = 5
        (0, 1, 0, 0, 12, 2, 3, 8, 9),
        (0, 1, 1, 0, 4, 2, 3, 8, 9),
        (2, 2, 1, 0, 70, 60, 62, 0, 1),            # s1 = T
        (1, 0, 0, 3, 9, 4, 5, 6, 7),               # dead
        (2, 0, 2, 0, 64, 63, 64, 1, 2),            # ends at t = 64
        (3, 1, 0, 0, 10, 2, 3, 4, 5),              # live, but entity 3 >= n_valid = 3 (< N = 5): padding, contributes nothing
        (1, 4, 1, 0, 6, 2, 3, 4, 5),               # the same on the column side
    ], 3, seed=3, n_rel=n_rel)
    return [d0, d1, d2], 5, 3, 70


def t1():
    d0 = doc(3, 1, [(0, 1, 0, 0, 1, 0, 1, 0, 1), (0, 1, 1, 0, 1, 3, 4, -5, -4),          # pair (0, 1): both slots live, divisor 1e-10
                    (1, 2, 1, -3, 4, 5, 6, -2, -1), (2, 0, 0, 1, 3, 0, 1, 0, 1)], 2, seed=4)
    d1 = doc(3, 1, [(0, 0, 1, 0, 1, 0, 1, 0, 1), (2, 1, 0, 0, 9, 700, 701, 0, 1)], 2, seed=5)
    return [d0, d1], 3, 2, 1


def none_live():
    d0 = doc(3, 20, [(0, 1, 0, 1, 9, 2, 3, 4, 5), (1, 2, 1, 5, 20, 6, 7, 8, 9), (2, 2, 0, 0, 0, 1, 2, 3, 4)], 2, seed=6)
    d1 = doc(2, 12, [(0, 1, 2, 0, 5, 1, 2, 3, 4), (1, 0, 0, 3, 4, 1, 2, 3, 4)], 2, seed=7)   # (j = 2 >= S = 2: dropped)
    return [d0, d1], 3, 2, 20


BATCHES = {"hand": hand, "t1": t1, "none_live": none_live}


def dis2idx(d):
    d = min(max(int(d), 0), 1023)
    return 0 if d == 0 else min(10, d.bit_length())      # config/Config.py:106-116


def pos_id(k, a, b, dis_plus):
    if k < a:
        return dis_plus - dis2idx(a - k)
    if k > b:
        return dis_plus + dis2idx(k - b)
    return dis_plus


def dense_numpy(docs, N, S, T, dis_plus=10):
    """(sen, pos_h, pos_t) uint8 [B,N,N,S,T] as gcgcn_tensorise writes them (csrc/tensorise.hip)."""
    B = len(docs)
    sen, ph, pt = (np.zeros((B, N, N, S, T), np.uint8) for _ in range(3))
    for b, d in enumerate(docs):
        for u, v, j, s0, s1, h0, h1, t0, t1 in d.slots.tolist():
            if u >= N or v >= N or j >= S:
                continue
            for k in range(max(s0, 0), min(s1, T)):
                sen[b, u, v, j, k] = 1
                ph[b, u, v, j, k] = pos_id(k, h0, h1, dis_plus) & 0xFF
                pt[b, u, v, j, k] = pos_id(k, t0, t1, dis_plus) & 0xFF
    return sen, ph, pt
