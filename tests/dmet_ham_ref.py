"""
numpy restatement of what routine/slater.py:1716-1778 and routine/slater_helper.py:183-270 of the reference compute, written as the
reference's own mask loops (NOT as the closed forms the device uses), so that the two can disagree:

  h1_scaled / h2_scaled_s4 / h2_scaled_s1   in-place class loops: imp-env blocks multiplied, env-env ASSIGNED zero (4-fold and
                                            one-body) or multiplied by 0.0 (1-fold)
  h2_scaled                                 every (in, out) storage pair of dmk_dmet_h2_scaled, padded pitches included
  rho_glob_R                                the literal loop over all cells R of the democratic global density
  restore_1 / to_s4 / pack_s8               storage conversions (ao2mo.restore)

Checked against the reference itself through tests/golden/G41_dmet_ham.npz (tests/test_dmet_ham_oracle.py); the checker of the
device code (tests/test_gpu_dmet_ham.py) where the fixture cannot reach: larger n, padded pitch, NaN / Inf.
"""
import itertools
import numpy as np


def tril_pairs(n):
    """(k, l) of every packed pair index, k >= l, in packed order."""
    return np.tril_indices(n)


def h1_scaled(H1, imp_idx):
    """(spin, n, n), in place."""
    n = H1.shape[-1]
    imp = np.asarray(imp_idx, dtype=int)
    env = np.asarray([i for i in range(n) if i not in set(imp.tolist())], dtype=int)
    for s in range(H1.shape[0]):
        H1[s][np.ix_(imp, env)] *= 0.5
        H1[s][np.ix_(env, imp)] *= 0.5
        H1[s][np.ix_(env, env)] = 0.0
    return H1


def pair_classes(n, imp_idx):
    """Number of impurity indices (0, 1, 2) of every packed pair."""
    k, l = tril_pairs(n)
    m = np.isin(np.arange(n), np.asarray(imp_idx, dtype=int))
    return m[k].astype(int) + m[l].astype(int)


def h2_scaled_s4(blk, n, imp_idx):
    """One 4-fold block (npair rows; columns beyond npair are padding and stay), in place: the nine (row class, column class)
    selections, class sum 4 skipped, class sum 0 assigned zero, the others multiplied by class sum / 4."""
    npair = n * (n + 1) // 2
    cls = pair_classes(n, imp_idx)
    sel = [np.where(cls == c)[0] for c in range(3)]
    view = blk[:, :npair]
    for a, b in itertools.product(range(3), repeat=2):
        if a + b == 4:
            continue
        mesh = np.ix_(sel[a], sel[b])
        if a + b == 0:
            view[mesh] = 0.0
        else:
            view[mesh] *= (a + b) * 0.25
    return blk


def h2_scaled_s1(blk, n, imp_idx):
    """One 1-fold block (n, n, n, n), in place: the sixteen (env | imp)^4 selections, each MULTIPLIED by (count of imp) / 4."""
    imp = np.asarray(imp_idx, dtype=int)
    env = np.asarray([i for i in range(n) if i not in set(imp.tolist())], dtype=int)
    sets = (env, imp)
    with np.errstate(invalid="ignore"):
        for c in itertools.product(range(2), repeat=4):
            blk[np.ix_(*[sets[x] for x in c])] *= sum(c) * 0.25
    return blk


def restore_1(e4, n):
    """4-fold (npair, npair) -> (n, n, n, n)."""
    idx = np.zeros((n, n), dtype=int)
    k, l = tril_pairs(n)
    idx[k, l] = idx[l, k] = np.arange(len(k))
    return e4[idx.reshape(-1)[:, None], idx.reshape(-1)[None, :]].reshape(n, n, n, n)


def to_s4(e, n, sym):
    """1-fold (n^4) or 8-fold (packed lower triangle of the 4-fold matrix) -> 4-fold."""
    npair = n * (n + 1) // 2
    if sym == 1:
        k, l = tril_pairs(n)
        return np.ascontiguousarray(e.reshape(n, n, n, n)[k[:, None], l[:, None], k[None, :], l[None, :]])
    out = np.empty((npair, npair))
    p, q = np.tril_indices(npair)
    out[p, q] = out[q, p] = e
    return out


def pack_s8(e4):
    return np.ascontiguousarray(e4[np.tril_indices(e4.shape[0])])


def h2_scaled(inp, n, imp_idx, in_sym, out_sym, ld_in=None, ld_out=None, out_fill=np.nan):
    """What dmk_dmet_h2_scaled writes: `inp` is the flat input buffer (rows of pitch ld_in for 4- and 1-fold storage), the result
    the flat output buffer with pitch ld_out, its padding = out_fill."""
    npair, nn = n * (n + 1) // 2, n * n
    row = {1: nn, 4: npair}
    if in_sym == 8:
        e = np.array(inp, dtype=np.float64)
    else:
        ld_in = row[in_sym] if ld_in is None else ld_in
        buf = np.asarray(inp, dtype=np.float64)
        e = np.empty((row[in_sym], ld_in))
        e.reshape(-1)[:(row[in_sym] - 1) * ld_in + row[in_sym]] = buf[:(row[in_sym] - 1) * ld_in + row[in_sym]]
        e = np.array(e[:, :row[in_sym]])
    if in_sym == 1 and out_sym == 1:
        res = h2_scaled_s1(e.reshape(n, n, n, n), n, imp_idx).reshape(nn, nn)
    else:
        e4 = e if in_sym == 4 else to_s4(e, n, in_sym)
        e4 = h2_scaled_s4(e4, n, imp_idx)
        res = e4 if out_sym == 4 else restore_1(e4, n).reshape(nn, nn)
    ld_out = row[out_sym] if ld_out is None else ld_out
    out = np.full((row[out_sym], ld_out), out_fill)
    out[:, :row[out_sym]] = res
    return out.reshape(-1)[:(row[out_sym] - 1) * ld_out + row[out_sym]]


# ---- global density ---------------------------------------------------------------------------------------------------------

def mesh_subtract(mesh):
    """sub[i][j] = index of cell i - cell j on a periodic mesh, cells in row-major order."""
    mesh = [int(m) for m in mesh] + [1] * (3 - len(mesh))
    cells = np.array(list(itertools.product(*[range(m) for m in mesh])))
    index = {tuple(c): i for i, c in enumerate(cells)}
    nc = len(cells)
    return np.array([[index[tuple((cells[i] - cells[j]) % np.array(mesh))] for j in range(nc)] for i in range(nc)])


def expand(stripe, sub):
    """(spin, ncells, n, n) stripe -> (spin, ncells n, ncells n): block (R1, R2) = stripe[R1 - R2]."""
    spin, nc, n, _ = stripe.shape
    return np.ascontiguousarray(stripe[:, sub].transpose(0, 1, 3, 2, 4)).reshape(spin, nc * n, nc * n)


def rho_glob_R(basis, sub, imp_idx, rho_emb, compact=True, cells=None):
    """The loop over all cells R (one fragment): the basis of cell R's impurity problem is `basis` with its cell blocks permuted
    by I -> I - R; its density C rho C^H gets the imp-env blocks halved and the env-env block zeroed, and the results are summed.
    basis (spin, ncells, nlo, neo), rho_emb (spin, neo, neo); `cells`: only these R (a partial sum, for timing the loop)."""
    spin, nc, nlo, neo = basis.shape
    ncol = nlo if compact else nc * nlo
    out = np.zeros((spin, nc * nlo, ncol))
    allrow = np.arange(nc * nlo)
    for R in (range(nc) if cells is None else cells):
        shifted = basis[:, [sub[I][R] for I in range(nc)]]
        imp = np.asarray(imp_idx, dtype=int) + R * nlo
        if not compact:
            imp = imp % (nc * nlo)
        env = allrow[~np.isin(allrow, imp)]
        in_cols = np.isin(np.arange(ncol), imp)
        imp_c, env_c = np.where(in_cols)[0], np.where(~in_cols)[0]
        for s in range(spin):
            C = shifted[s].reshape(nc * nlo, neo)
            d = C.dot(rho_emb[s]).dot(C[:ncol].conj().T)
            d[np.ix_(imp, env_c)] *= 0.5
            d[np.ix_(env, imp_c)] *= 0.5
            d[np.ix_(env, env_c)] = 0.0
            out[s] += d
    return out.reshape(spin, nc, nlo, nlo) if compact else out
