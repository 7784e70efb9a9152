"""
CPU checks of the code behind the solver: the numpy restatement tests/dmet_ham_ref.py reproduces what the
reference itself computed (golden G41, tools/gen_golden_dmet_ham.py), the pure-numpy get_H1_scaled of this package does so bit for
bit, and the new entry points are part of the rebinding plan.  No device code runs here.
"""
import importlib
import os

import numpy as np
import pytest

from tests import dmet_ham_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["uhf_231", "rhf_411", "uhf_222"]
SLATER_NAMES = ["get_H1_scaled", "get_H2_scaled", "transformResults", "get_veff_from_rdm1_emb", "get_H_dmet", "get_E_dmet",
                "get_E_dmet_HF", "get_H1_dmet"]
HELPER_NAMES = ["get_emb_basis_other_cell", "get_rho_glob_R", "get_rho_glob_k", "get_rho_glob_full"]


@pytest.fixture(scope="module")
def g41():
    return np.load(os.path.join(GOLD, "G41_dmet_ham.npz"))


@pytest.fixture(scope="module")
def g8():
    return np.load(os.path.join(GOLD, "G8_embham.npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_of_the_scalers_reproduces_the_reference(g41, g8, name):
    imp, H2 = g41[name + "/imp_idx"], g8[name + "/H2"]
    nb = g41[name + "/basis"].shape[-1]
    assert np.array_equal(ref.h1_scaled(np.array(g41[name + "/H1"]), imp), g41[name + "/H1_scaled"])
    for s in range(H2.shape[0]):
        want4 = g41[name + "/H2_scaled_s4"][s]
        assert np.array_equal(ref.h2_scaled_s4(np.array(H2[s]), nb, imp), want4)
        assert np.array_equal(ref.h2_scaled(H2[s].reshape(-1), nb, imp, 4, 4), want4.reshape(-1))
        if np.array_equal(H2[s], H2[s].T):          # (the alpha-beta block has no 8-fold form)
            assert np.array_equal(ref.to_s4(ref.pack_s8(H2[s]), nb, 8), H2[s])
            assert np.array_equal(ref.h2_scaled(ref.pack_s8(H2[s]), nb, imp, 8, 4), want4.reshape(-1))
        e1 = ref.restore_1(H2[s], nb)
        assert np.array_equal(ref.to_s4(e1, nb, 1), H2[s])
        assert np.array_equal(ref.h2_scaled(e1.reshape(-1), nb, imp, 1, 4), want4.reshape(-1))
        if name + "/H2_scaled_s1" in g41.files:
            want1 = g41[name + "/H2_scaled_s1"][s]
            assert np.array_equal(ref.h2_scaled_s1(np.array(e1), nb, imp), want1)
            assert np.array_equal(ref.h2_scaled(e1.reshape(-1), nb, imp, 1, 1), want1.reshape(-1))
            assert np.array_equal(ref.h2_scaled(H2[s].reshape(-1), nb, imp, 4, 1), want1.reshape(-1))


def test_restatement_with_padded_pitch_and_the_two_zero_rules():
    n, imp = 5, [0, 2, 4]
    npair = n * (n + 1) // 2
    rng = np.random.default_rng(5)
    e4 = rng.standard_normal((npair, npair))
    e4 = e4 + e4.T
    buf = np.full((npair, npair + 3), 7.0)
    buf[:, :npair] = e4
    got = ref.h2_scaled(buf.reshape(-1), n, imp, 4, 4, ld_in=npair + 3, ld_out=npair + 2, out_fill=-1.0)
    got = np.concatenate([got, [-1.0, -1.0]]).reshape(npair, npair + 2)
    assert np.array_equal(got[:, :npair], ref.h2_scaled_s4(np.array(e4), n, imp)) and np.all(got[:-1, npair:] == -1.0)
    # a NaN in an element without impurity index: assigned zero in the 4-fold form, kept by the 1-fold form's multiplication
    cls = ref.pair_classes(n, imp)
    p0 = int(np.where(cls == 0)[0][0])
    e4n = np.array(e4)
    e4n[p0, p0] = np.nan
    assert ref.h2_scaled_s4(np.array(e4n), n, imp)[p0, p0] == 0.0
    k, l = (int(x[p0]) for x in ref.tril_pairs(n))
    assert np.isnan(ref.h2_scaled_s1(ref.restore_1(e4n, n).copy(), n, imp)[k, l, k, l])


@pytest.mark.parametrize("name", CASES)
def test_restatement_of_the_cell_loop_reproduces_the_reference(g41, name):
    basis, rho, imp = g41[name + "/basis"], g41[name + "/rdm1_emb"], g41[name + "/lo_imp_idx"]
    nk = basis.shape[1]
    mesh = {6: (2, 3, 1), 4: (4, 1, 1), 8: (2, 2, 2)}[nk]
    sub = ref.mesh_subtract(mesh)
    stripe = ref.rho_glob_R(basis, sub, imp, rho)
    assert np.abs(stripe - g41[name + "/rho_glob_R"]).max() < 1e-12
    assert np.abs(ref.rho_glob_R(basis, sub, imp, rho, compact=False) - g41[name + "/rho_glob_R_full"]).max() < 1e-12
    # the full forms are the expanded stripe (what the device path relies on), and the signed two-fragment sum is linear
    assert np.abs(ref.expand(stripe, sub) - g41[name + "/rho_glob_full"]).max() < 1e-12
    assert np.abs(ref.expand(stripe, sub) - g41[name + "/rho_glob_R_full"]).max() < 1e-12
    two = ref.expand(stripe, sub) - ref.expand(ref.rho_glob_R(basis, sub, g41[name + "/frag2_imp_idx"], g41[name + "/rdm1_emb2"]), sub)
    assert np.abs(two - g41[name + "/rho_glob_2frag"]).max() < 1e-12


@pytest.mark.parametrize("name", CASES)
def test_get_H1_scaled_is_the_reference_bit_for_bit(g41, name):
    from libdmet_preview_amd.routine import slater
    H1 = np.array(g41[name + "/H1"])
    out = slater.get_H1_scaled(H1, g41[name + "/imp_idx"])
    assert out is H1 and np.array_equal(out, g41[name + "/H1_scaled"])


def test_new_entry_points_are_in_the_binding_table():
    from libdmet_preview_amd import patch
    table = set(patch.binding_table())
    for name in SLATER_NAMES:
        assert ("routine.slater", "routine.slater", name) in table, name
    for name in HELPER_NAMES:
        for holder in ("routine.slater_helper", "routine.slater"):
            assert ("routine.slater_helper", holder, name) in table, (holder, name)
    for ours, _, name in table:
        if name in SLATER_NAMES + HELPER_NAMES:
            assert callable(getattr(importlib.import_module("libdmet_preview_amd." + ours), name))
    # routine.slater star-imports its helper module, as the reference does: one object under both names
    from libdmet_preview_amd.routine import slater, slater_helper
    for name in HELPER_NAMES:
        assert getattr(slater, name) is getattr(slater_helper, name)
