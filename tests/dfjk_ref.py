"""
numpy restatement of the density-fitted k-point J/K build, one DF block at a time (no eri_7d is ever formed):

  rho[s][L]     = sum_k sum_pq B^(k,k)[L,p,q] dm[s,k][q,p]
  vj[s,k][r,t]  = (1/nk) sum_L rho[s][L] B^(k,k)[L,r,t]
  vk[s,ki][p,t] = (1/nk) sum_kj sum_L sum_qr B^(ki,kj)[L,p,q] dm[s,kj][q,r] conj(B^(ki,kj)[L,t,r])
  exxdiv='ewald': vk[s,k] += madelung S[k] dm[s,k] S[k]

Checked against the reference's get_jk_from_eri_7d through tests/golden/G39_dfjk.npz (tests/test_dfjk_oracle.py); the checker
of the device build (tests/test_gpu_dfjk.py).  `block(i, j)` returns the (naux, nao, nao) block of the ordered pair.
"""
import numpy as np


def get_jk(block, dm, with_j=True, with_k=True, madelung=None, ovlp=None, ki_list=None):
    dm = np.asarray(dm, dtype=np.complex128)
    old_shape = dm.shape
    if dm.ndim == 3:
        dm = dm[None]
    spin, nk, nao, _ = dm.shape
    vj = vk = None
    if with_j:
        rho = 0.0
        for k in range(nk):
            rho = rho + np.einsum("Lpq,sqp->sL", np.asarray(block(k, k)), dm[:, k])
        vj = np.zeros(dm.shape, dtype=np.complex128)
        for k in range(nk):
            vj[:, k] = np.einsum("sL,Lrt->srt", rho, np.asarray(block(k, k))) / nk
        vj = vj.reshape(old_shape)
    if with_k:
        vk = np.zeros(dm.shape, dtype=np.complex128)
        for ki in (range(nk) if ki_list is None else ki_list):
            for kj in range(nk):
                B = np.asarray(block(ki, kj))
                for s in range(spin):
                    W = np.matmul(B, dm[s, kj])                                          # (L, p, r)
                    vk[s, ki] += np.tensordot(W, B.conj(), axes=([0, 2], [0, 2]))        # (p, t)
            vk[:, ki] /= nk
            if madelung is not None:
                S = np.asarray(ovlp[ki])
                for s in range(spin):
                    vk[s, ki] += madelung * S.dot(dm[s, ki]).dot(S)
        vk = vk.reshape(old_shape)
    return vj, vk


def expand_pairs(stored, nk):
    """All nk^2 blocks from the i <= j ones by the pair relation B^(j,i)[L,r,t] = conj(B^(i,j)[L,t,r])."""
    blocks = {}
    for i in range(nk):
        for j in range(i, nk):
            b = np.asarray(stored[(i, j)])
            blocks[(i, j)] = b
            if i != j:
                blocks[(j, i)] = np.ascontiguousarray(b.conj().transpose(0, 2, 1))
    return blocks


def stripe_blocks(mesh, nao, naux, seed):
    """Blocks with the pair relation AND time-reversal symmetry, from a real tensor T[R,S,L,p,q] with T[S,R,L,q,p] = T[R,S,L,p,q]:
    B^(i,j) = sum_RS T[R,S] exp(-i k_i.R) exp(+i k_j.S).  Returns (scaled k-points, {(i, j): block})."""
    rng = np.random.default_rng(seed)
    mesh = tuple(int(m) for m in mesh)
    nk = int(np.prod(mesh))
    cells = np.array([[a, b, c] for a in range(mesh[0]) for b in range(mesh[1]) for c in range(mesh[2])])
    ks = np.array([[a, b, c] for a in np.fft.fftfreq(mesh[0]) for b in np.fft.fftfreq(mesh[1]) for c in np.fft.fftfreq(mesh[2])])
    T = rng.standard_normal((nk, nk, naux, nao, nao)) / nao
    T = 0.5 * (T + T.transpose(1, 0, 2, 4, 3))
    ph = np.exp(-2j * np.pi * ks.dot(cells.T))                  # [k, R]
    blocks = {}
    for i in range(nk):
        for j in range(nk):
            blocks[(i, j)] = np.ascontiguousarray(np.einsum("R,S,RSLpq->Lpq", ph[i], ph[j].conj(), T))
    return ks, blocks


def stripe_density(mesh, nao, spin, seed):
    """dm[s,k] = sum_R D[s,R] exp(-i k.R) from a real stripe with D[-R] = D[R]^T: Hermitian at every k, dm[-k] = conj(dm[k])."""
    rng = np.random.default_rng(seed)
    mesh = tuple(int(m) for m in mesh)
    nk = int(np.prod(mesh))
    cells = np.array([[a, b, c] for a in range(mesh[0]) for b in range(mesh[1]) for c in range(mesh[2])])
    ks = np.array([[a, b, c] for a in np.fft.fftfreq(mesh[0]) for b in np.fft.fftfreq(mesh[1]) for c in np.fft.fftfreq(mesh[2])])
    neg = [int(np.where((((-cells[r]) % np.array(mesh)) == cells).all(axis=1))[0][0]) for r in range(nk)]
    D = rng.standard_normal((spin, nk, nao, nao))
    D = 0.5 * (D + D[:, neg].transpose(0, 1, 3, 2))
    ph = np.exp(-2j * np.pi * ks.dot(cells.T))
    return np.einsum("kR,sRpq->skpq", ph, D)
