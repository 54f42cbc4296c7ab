"""numpy restatement of the time-correlation sampler's contract (include/aztot.h, 'time correlation functions'): per-atom terms, the fixed summation
tree, the ring of origins and the accumulators.  Every operation is one IEEE fp64 operation on arrays, so the results can be compared bit for bit."""
import numpy as np

CHUNK, RUN = 256, 64


def fold(a):
    """fold the last axis (a power of two long) by halving: a[j] = a[j] + a[j + h] for h = len / 2 ... 1"""
    h = a.shape[-1] // 2
    while h >= 1:
        a = a[..., :h] + a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def tree_levels(n):
    """additions on the path of one term: 6 in its run, 2 in its chunk, log2 of the padded chunk count"""
    chunks = max(1, -(-n // CHUNK))
    return 6 + 2 + int(np.ceil(np.log2(chunks)))


def tree_sum(t):
    """the sum of the contract: runs of 64 ids, the four runs of a chunk of 256, the chunks padded to a power of two"""
    t = np.asarray(t, dtype=np.float64)
    chunks = max(1, -(-t.size // CHUNK))
    a = np.zeros(chunks * CHUNK)
    a[:t.size] = t
    w = fold(a.reshape(chunks, CHUNK // RUN, RUN))          # [chunk][run]
    c = (w[:, 0] + w[:, 2]) + (w[:, 1] + w[:, 3])
    pad = 1
    while pad < chunks:
        pad *= 2
    p = np.zeros(pad)
    p[:chunks] = c
    return float(fold(p))


def min_image(d, L):
    """delta_periodic (box.cpp:180-205)"""
    return np.where(d > 0.5 * L, d - L, np.where(d < -0.5 * L, d + L, d))


def terms(cur, org, box):
    """(m_i, v_i) of every atom: cur / org are dicts of x y z vx vy vz"""
    d = [min_image(cur[k] - org[k], box[a]) for a, k in enumerate("xyz")]
    m = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    v = (cur["vx"] * org["vx"] + cur["vy"] * org["vy"]) + cur["vz"] * org["vz"]
    return m, v


def species_sums(term, types, n_species):
    return [tree_sum(np.where(types == s, term, 0.0)) for s in range(n_species)]


class Sampler:
    """ring of M origins, one every E samples; accumulators per lag.  `pairs` lists every (sample, origin) correlated so far"""

    def __init__(self, n_origins, origin_every, types, n_species, box):
        self.M, self.E = int(n_origins), int(origin_every)
        self.types, self.ns, self.box = np.asarray(types), int(n_species), [float(b) for b in box]
        self.n_lags = self.M * self.E
        self.number = np.array([int((self.types == s).sum()) for s in range(self.ns)], dtype=np.int64)
        self.reset()

    def reset(self):
        self.samples = 0
        self.ring = [None] * self.M             # (origin's sample number, state)
        self.count = np.zeros(self.n_lags, dtype=np.int64)
        self.msd = np.zeros((self.n_lags, self.ns))
        self.vaf = np.zeros((self.n_lags, self.ns))
        self.pairs = []

    def sample(self, state=None):
        c = self.samples
        cur = None if state is None else {k: np.array(state[k], dtype=np.float64) for k in ("x", "y", "z", "vx", "vy", "vz")}
        if c % self.E == 0:
            self.ring[(c // self.E) % self.M] = (c, cur)
        for slot in range(self.M):
            if self.ring[slot] is None:
                continue
            o, org = self.ring[slot]
            lag = c - o
            self.pairs.append((c, o))
            self.count[lag] += 1
            if cur is not None:
                m, v = terms(cur, org, self.box)
                self.msd[lag] = self.msd[lag] + np.array(species_sums(m, self.types, self.ns))
                self.vaf[lag] = self.vaf[lag] + np.array(species_sums(v, self.types, self.ns))
        self.samples += 1

    def values(self):
        w = (self.count[:, None] * self.number[None, :]).astype(np.float64)
        ok = w != 0.0
        safe = np.where(ok, w, 1.0)
        return np.where(ok, self.msd / safe, 0.0), np.where(ok, self.vaf / safe, 0.0)
