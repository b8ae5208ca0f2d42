"""Helpers of the compact-mode PNG tests (tests/helpers/png_check.py stays as it is): the block type each stripe starts with, and the
histograms on which png_code_lengths is checked, with the three properties every result must have."""
import heapq

import numpy as np

import png_check as pc


def btypes(data: bytes):
    """BTYPE (0 stored, 1 fixed, 2 dynamic) of the first block of every stripe: the encoder writes one IDAT chunk per stripe (the first
    behind the two-byte zlib header) and a last one of four bytes that holds the Adler-32 alone"""
    idat = [body for typ, body in pc.chunks_of(data) if typ == b"IDAT"]
    assert len(idat) >= 2 and len(idat[-1]) == 4, [len(b) for b in idat]
    out = []
    for k, body in enumerate(idat[:-1]):
        first = body[2] if k == 0 else body[0]
        out.append((first >> 1) & 3)
    return out


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return np.array(f[:n], np.uint32)


def random_histograms(limit, count=200, seed=11):
    """seeded histograms for one limit (15: up to 286 symbols, 7: up to 19): flat, sparse and steep ones, every sum below 2^22.  The steep
    ones (geometric frequencies) have Huffman trees deeper than the limit"""
    rng = np.random.RandomState(seed + limit)
    nmax = 286 if limit == 15 else 19
    out = []
    for j in range(count):
        n = int(rng.randint(2, nmax + 1))
        kind = j % 4
        if kind == 0:
            f = rng.randint(0, 50, n)
        elif kind == 1:
            f = rng.randint(0, 3000, n) * (rng.rand(n) < 0.3)
        elif kind == 2:                      # geometric, ratio 1.5 .. 2.2, on up to 24 symbols; the rest small
            f = rng.randint(0, 3, n)
            m = min(n, int(rng.randint(2, 25)))
            idx = rng.permutation(n)[:m]
            f[idx] = np.minimum(1 << 16, np.floor(rng.uniform(1.5, 2.2) ** np.arange(m)) + 1).astype(np.int64)
        else:
            f = rng.randint(1, 4, n)
        f = np.asarray(f, np.int64)
        if np.count_nonzero(f) < 2:
            f[:2] = (1, 2)
        assert f.sum() < (1 << 22)
        out.append(f.astype(np.uint32))
    return out


def direct_histograms():
    """[(name, freq, limit)] of the issue's direct cases"""
    one = np.zeros(30, np.uint32)
    one[7] = 5
    two = np.zeros(30, np.uint32)
    two[3], two[29] = 9, 1
    return [("fib18", fibonacci(18), 15), ("fib10", fibonacci(10), 7), ("one", one, 15), ("two", two, 15),
            ("all286", np.full(286, 7, np.uint32), 15)]


def huffman(freq):
    """(optimal total cost, depth of heapq's tree) of the used symbols; the cost is unique, the depth is this tree's"""
    heap = [(int(f), 0) for f in freq if f]
    if len(heap) < 2:
        return sum(f for f, _ in heap), 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def check_lengths(freq, limit, lens, name=""):
    """zero exactly where the frequency is zero, nothing above the limit, Kraft sum exactly 1 (a lone symbol: the one-bit code, 1/2),
    and the optimum wherever heapq's tree fits the limit"""
    freq = np.asarray(freq, np.int64)
    lens = np.asarray(lens, np.int64)
    assert lens.shape == freq.shape
    assert np.array_equal(lens == 0, freq == 0), name
    assert lens.max() <= limit, (name, int(lens.max()))
    used = lens[lens > 0]
    kraft = int(np.sum(1 << (limit - used)))
    if len(used) == 1:
        assert used[0] == 1, name
        return
    assert kraft == 1 << limit, (name, kraft, 1 << limit)
    best, depth = huffman(freq)
    cost = int(np.sum(freq * lens))
    assert cost >= best, (name, cost, best)
    if depth <= limit:
        assert cost == best, (name, cost, best)
