"""What the pair-list builder (k_build_lists, csrc/pair_list.hip.h) promises, restated in numpy from box, grid, rMax, slack and positions alone
(tests/test_list_model.py, tests/test_gpu_pair_lists.py).

The promise: a rebuild leaves, for every atom, every atom within the LIST RADIUS rMax + 2 slack of it (minimum image) among its cell's
candidates, under the right periodic image code.  Between two rebuilds nobody moves farther than slack, so a pair that comes within rMax was
within the list radius at the rebuild: no pair inside the cut-off can be missing from a step's forces.

`geometry` restates the engine's rule for grid, skin and slack (Engine::choose_cells and the "lazy re-sort" block of Engine::construct), `Builder`
the kernel's f32 arithmetic: positions relative to the centre of the atom's own cell (one rounding to f32), a neighbour's position as that plus
whole cell edges, the pruning of candidates against the dilated bounding box of the cell's atoms, and the expanded-form filter
thr - |ri|^2 - |rj|^2 + 2 ri.rj >= 0 with the widened threshold `thrList`.  The matrix instruction's internal accumulation order is not
documented: the filter is evaluated both with every product and sum rounded to f32 in turn ('unfused') and with one rounding of the exact sum
('fused'); the builder's margin must cover both.  `exact_pairs` is the enumeration the lists are held to, `lj_forces` the longdouble force
reference of the GPU test.
"""
import numpy as np

LD = np.longdouble
F32 = np.float32
OFFSETS26 = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def geometry(box, r_max, cell_list=0.0, skin=0.0):
    """Grid, stencil, slack and list radius the engine chooses on one GPU for options.skin = `skin` (0: automatic) and control.cell_list = `cell_list`."""
    box = [float(v) for v in box]
    size = cell_list if cell_list > 0 else r_max
    target = skin if skin > 0 else min(0.5, max(0.15, 0.036 * r_max))
    if 0.95 * r_max <= size < r_max + target:
        if not any(int(np.floor(L / (r_max + target))) < 5 <= int(np.floor(L / size)) for L in box):
            size = r_max + target
    nc = [min(1024, max(1, int(np.floor(L / size)))) for L in box]
    csz = [L / n for L, n in zip(box, nc)]
    hw = [max(0, int(np.ceil(r_max / c - 1e-12))) for c in csz]
    slack = min(0.49 * (h * c - r_max) for h, c in zip(hw, csz))
    lazy = all(n >= 2 * (h + 1) + 1 for n, h in zip(nc, hw)) and slack > 1e-3
    slack = min(slack, 0.5 * 1.25 * target) if lazy else 0.0
    r_list = r_max + 2.0 * slack
    return dict(box=box, nc=nc, csz=csz, icsz=[n / L for L, n in zip(box, nc)], hw=hw, slack=slack, skin=2.0 * slack, lazy=lazy, r_max=float(r_max),
                r_list=r_list, prune_r2=r_list * r_list * (1.0 + 1e-12), n_cells=nc[0] * nc[1] * nc[2])


def cell_coords(pos, g):
    """(N, 3) integer cell coordinates: floor(x * n / L) in fp64, folded into the grid (cell_coord, csrc/kernels.hip.h)"""
    c = np.floor(np.asarray(pos, dtype=np.float64) * np.asarray(g["icsz"])).astype(np.int64)
    return np.mod(c, np.asarray(g["nc"]))


def cell_index(cc, g):
    return (cc[:, 0] * g["nc"][1] + cc[:, 1]) * g["nc"][2] + cc[:, 2]


def populations(pos, g):
    """atoms per cell, all cells"""
    return np.bincount(cell_index(cell_coords(pos, g), g), minlength=g["n_cells"])


def rel_f32(pos, cc, g):
    """position relative to the centre of the atom's own cell, rounded once to f32 (k_rank_gather: PairLists::rel)"""
    csz = np.asarray(g["csz"])
    return (np.asarray(pos, dtype=np.float64) - (cc * csz + 0.5 * csz)).astype(F32)


def min_image(d, box):
    box = np.asarray(box, dtype=d.dtype)
    return d - box * np.rint(d / box)


def exact_pairs(pos, box, radius, dtype=LD):
    """(i, j, r2) of all unordered pairs i < j with minimum-image distance <= radius, decided in `dtype` (periodic KD-tree for the candidates)"""
    from scipy.spatial import cKDTree
    box64 = np.asarray(box, dtype=np.float64)
    p = np.mod(np.asarray(pos, dtype=np.float64), box64)
    p[p >= box64] = 0.0
    ij = cKDTree(p, boxsize=box64).query_pairs(radius * (1.0 + 1e-9) + 1e-9, output_type="ndarray")
    ij = ij[np.lexsort((ij[:, 1], ij[:, 0]))]
    P = np.asarray(pos, dtype=dtype)
    d = min_image(P[ij[:, 0]] - P[ij[:, 1]], box)
    r2 = (d * d).sum(1)
    keep = r2 <= dtype(radius) * dtype(radius)
    return ij[keep, 0], ij[keep, 1], r2[keep]


def lj_term(eps, sigma, r2):
    """(f, S_F) of Lennard-Jones in longdouble: f = -(1/r) dU/dr = 24 eps / r^2 (2 s^12 - s^6), S_F the sum of the absolute values of its terms
    (tests/pair_reference.py vdw kind 1)"""
    r2 = np.asarray(r2, dtype=LD)
    s6 = (LD(sigma) * LD(sigma) / r2) ** 3
    a = LD(24.0) * LD(eps) / r2
    return a * (LD(2.0) * s6 * s6 - s6), abs(a) * (LD(2.0) * s6 * s6 + s6)


def lj_forces(pos, types, box, vdw, r_max):
    """Per-atom force and tolerance scale of the exact enumeration, in longdouble, at positions `pos`.
    vdw: {(ta, tb): (eps, sigma, rc)} for the species pairs with a potential (both orders looked up).  Returns dict(F (N, 3), scale (N,): sum_j S_F r,
    smallest (N,): the smallest single |f| r among the atom's pairs (inf without any), i, j, r2: the pairs inside their cut-off, near: how many
    pairs sit within 1e-12 (relative) of their cut-off - such a pair could be decided either way in fp64)."""
    N = len(types)
    i, j, r2 = exact_pairs(pos, box, r_max * (1.0 + 1e-9))
    P = np.asarray(pos, dtype=LD)
    d = min_image(P[i] - P[j], box)
    F = np.zeros((N, 3), dtype=LD)
    scale = np.zeros(N, dtype=LD)
    smallest = np.full(N, np.inf, dtype=LD)
    keep = np.zeros(len(i), dtype=bool)
    near = 0
    ti, tj = np.asarray(types)[i], np.asarray(types)[j]
    for (a, b), (eps, sigma, rc) in vdw.items():
        if a > b:
            continue
        m = ((ti == a) & (tj == b)) | ((ti == b) & (tj == a))
        rc2 = LD(rc) * LD(rc)
        near += int((m & (abs(r2 / rc2 - 1) < LD(2e-12))).sum())
        m &= r2 <= rc2
        f, sf = lj_term(eps, sigma, r2[m])
        r = np.sqrt(r2[m])
        fd = f[:, None] * d[m]
        for k in range(3):
            np.add.at(F[:, k], i[m], fd[:, k])
            np.add.at(F[:, k], j[m], -fd[:, k])
        for idx in (i[m], j[m]):
            np.add.at(scale, idx, sf * r)
            np.minimum.at(smallest, idx, abs(f) * r)
        keep |= m
    return dict(F=F, scale=scale, smallest=smallest, i=i[keep], j=j[keep], r2=r2[keep], near=near)


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_widening", "tight_box", "wrong_image")


class Builder:
    """The lists a rebuild at positions `pos` leaves, cell by cell.  `mutation` (None or one of MUTATIONS) breaks one of the builder's margins:
      no_widening   thrList without its error-bound term and the pruning radius at rMax instead of the list radius
      tight_box     the bounding box without its dilation and shrunk by one f32 ulp of the cell edge, the pruning radius without the 1e-5 it
                    carries for the rounding of the coordinates (that allowance is 80 times the dilation: with it in place the box cannot lose anything)
      wrong_image   candidates across the upper x wall get image code 1 (no shift) instead of 2
    """

    def __init__(self, pos, g, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.g, self.mutation = g, mutation
        self.pos = np.asarray(pos, dtype=np.float64)
        self.cc = cell_coords(self.pos, g)
        self.cell = cell_index(self.cc, g)
        self.rel = rel_f32(self.pos, self.cc, g)
        order = np.lexsort((np.arange(len(self.cell)), self.cell))          # by cell, by id inside a cell (k_rank_gather ranks by id)
        self.order = order
        self.start = np.searchsorted(self.cell[order], np.arange(g["n_cells"] + 1))
        self.cs = [F32(c) for c in g["csz"]]
        r_list2 = g["r_max"] ** 2 if mutation == "no_widening" else g["prune_r2"]
        self.prune_f = F32(r_list2 * (1.0 if mutation == "tight_box" else 1.0 + 1e-5))
        h = [0.5 * c for c in g["csz"]]
        rl = np.sqrt(g["prune_r2"])
        ext2 = sum((hk + rl) ** 2 for hk in h)
        self.thr = F32(r_list2 + (0.0 if mutation == "no_widening" else 1.9073486328125e-06 * (4.0 * ext2 + g["prune_r2"])))
        self._built = None

    def atoms_of(self, c):
        return self.order[self.start[c]:self.start[c + 1]]

    def box_of(self, rel):
        """centre and half-widths of the bounding box of a cell's atoms (f32, as the kernel forms them)"""
        lo, hi = rel.min(0), rel.max(0)
        bc = F32(0.5) * (lo + hi)
        bh = F32(0.5) * (hi - lo)
        if self.mutation == "tight_box":
            return bc, bh - np.array([np.spacing(c) for c in self.cs], dtype=F32)
        return bc, bh * F32(1.000001) + F32(1e-5)

    def candidates(self, c):
        """(atom, image code (3,), position relative to this cell's centre (f32)) of the cell's candidates, stencil order"""
        g = self.g
        nc, hw = g["nc"], g["hw"]
        cx, rem = divmod(c, nc[1] * nc[2])
        cy, cz = divmod(rem, nc[2])
        mine = self.atoms_of(c)
        bc, bh = self.box_of(self.rel[mine])
        rng = [np.arange(-h, h + 1) if 2 * h + 1 <= n else np.arange(-h, -h + n) for h, n in zip(hw, nc)]
        off = np.stack(np.meshgrid(*rng, indexing="ij"), -1).reshape(-1, 3)             # x slowest, z fastest: the order the kernel stages in
        to = off + np.array([cx, cy, cz])
        n3 = np.array(nc)
        img = 1 + (to >= n3) - (to < 0)
        if self.mutation == "wrong_image":
            img[img[:, 0] == 2, 0] = 1
        to = np.mod(to, n3)
        cell = (to[:, 0] * nc[1] + to[:, 1]) * nc[2] + to[:, 2]
        cnt = self.start[cell + 1] - self.start[cell]
        tot = int(cnt.sum())
        which = np.repeat(np.arange(len(cell)), cnt)
        at = self.order[np.repeat(self.start[cell], cnt) + np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
        r, o = self.rel[at], off[which]
        x = np.empty_like(r)
        x[:, 0] = r[:, 0] + o[:, 0].astype(F32) * self.cs[0]                            # product and sum each rounded to f32
        x[:, 1] = r[:, 1] + o[:, 1].astype(F32) * self.cs[1]
        x[:, 2] = (o[:, 2].astype(np.float64) * np.float64(self.cs[2]) + r[:, 2].astype(np.float64)).astype(F32)       # fmaf: one rounding
        d = np.maximum(np.abs(x - bc) - bh, F32(0))
        keep = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) <= self.prune_f
        return mine, at[keep], img[which][keep], x[keep]

    def filter(self, xi, xj, fused):
        """hit mask [atoms of the cell, candidates]: thr - |ri|^2 + sum_k A_k B_k >= 0 with A = (xj, yj, zj, -|rj|^2), B = (2 xi, 2 yi, 2 zi, 1)"""
        c_atom = self.thr - (xi[:, 0] * xi[:, 0] + xi[:, 1] * xi[:, 1] + xi[:, 2] * xi[:, 2])
        w = -(xj[:, 0] * xj[:, 0] + xj[:, 1] * xj[:, 1] + xj[:, 2] * xj[:, 2])
        a = np.concatenate([xj, w[:, None]], 1)                               # [cand, 4]  f32
        b = np.concatenate([F32(2) * xi, np.ones((len(xi), 1), dtype=F32)], 1)       # [atom, 4]  f32
        if fused:
            d = c_atom.astype(np.float64)[:, None] + (b.astype(np.float64)[:, None, :] * a.astype(np.float64)[None, :, :]).sum(-1)
            return d.astype(F32) >= 0
        d = np.repeat(c_atom[:, None], len(xj), 1)
        for k in range(4):
            d = d + b[:, None, k] * a[None, :, k]
        return d >= 0

    def build(self):
        """per non-empty cell: dict(atoms, cand, code, n_cand, hits {fused: mask})"""
        if self._built is None:
            out = {}
            for c in np.flatnonzero(np.diff(self.start) > 0):
                mine, at, code, x = self.candidates(c)
                xi = self.rel[mine]
                hits = {f: self.filter(xi, x, f) & (mine[:, None] != at[None, :]) for f in (False, True)}
                out[int(c)] = dict(atoms=mine, cand=at, code=code, n_cand=len(at), hits=hits)
            self._built = out
        return self._built

    def listed(self, fused):
        """(i, j, effective r) of every list entry: the distance k_pair_list would see, from the fp64 positions and the entry's image code"""
        I, J, R = [], [], []
        L = np.asarray(self.g["box"])
        for rec in self.build().values():
            a, b = np.nonzero(rec["hits"][fused])
            i, j = rec["atoms"][a], rec["cand"][b]
            d = self.pos[i] - (self.pos[j] + (rec["code"][b] - 1) * L)
            I.append(i); J.append(j); R.append(np.sqrt((d * d).sum(1)))
        return np.concatenate(I), np.concatenate(J), np.concatenate(R)

    def lost(self, i, j, r2, fused):
        """which of the exact pairs (i, j, r2: minimum-image) are NOT served by the lists in both directions (mask)"""
        li, lj, lr = self.listed(fused)
        N = len(self.pos)
        d = min_image(self.pos[li] - self.pos[lj], self.g["box"])
        dm = np.sqrt((d * d).sum(1))
        good = np.unique((li * N + lj)[np.abs(lr - dm) <= 1e-9 * dm])        # entries whose image code shows the partner where it is
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        return ~(np.isin(i * N + j, good) & np.isin(j * N + i, good))

    def candidate_counts(self):
        return {c: rec["n_cand"] for c, rec in self.build().items()}
