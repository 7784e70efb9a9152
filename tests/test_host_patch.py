"""
Host logic of libdmet_preview_amd.patch (the rebinding of SURVEY.md section 8b): every entry of the binding table
exists on our side; install / uninstall rebind every holder of a name and restore it; the table is checked against
the names of the reference's real module tree (golden G40, read off it under oracle/shim.py).  No compute is called.
"""
import importlib
import json
import os
import sys
import types

import pytest

from libdmet_preview_amd import patch


def test_binding_table_resolves_on_our_side():
    for ours, ref, name in patch.binding_table():
        mod = importlib.import_module("libdmet_preview_amd." + ours)
        assert callable(getattr(mod, name)), (ours, name)
    from libdmet_preview_amd.system.lattice import Lattice
    for name in patch._LATTICE_METHODS:
        assert callable(getattr(Lattice, name))


def _fake_reference(root):
    """A module tree with the reference's module names whose attributes are placeholders."""
    mods = {}

    def mk(name):
        m = types.ModuleType(name)
        sys.modules[name] = m
        mods[name] = m
        return m
    mk(root)
    for ours, ref, name in patch.binding_table():
        parts = ref.split(".")
        for i in range(1, len(parts) + 1):
            full = root + "." + ".".join(parts[:i])
            if full not in mods:
                mk(full)
        setattr(mods[root + "." + ref], name, ("placeholder", ref, name))
    lat = mods.get(root + ".system.lattice") or mk(root + ".system.lattice")

    class Lattice(object):
        pass
    for name in patch._LATTICE_METHODS:
        setattr(Lattice, name, ("placeholder", name))
    lat.Lattice = Lattice
    return mods


def test_install_rebinds_every_holder_and_uninstall_restores():
    root = "fake_libdmet_for_patch_test"
    mods = _fake_reference(root)
    try:
        handle = patch.install(reference_package=root)
        for ours, ref, name in patch.binding_table():
            mine = getattr(importlib.import_module("libdmet_preview_amd." + ours), name)
            assert getattr(mods[root + "." + ref], name) is mine, (ref, name)
        from libdmet_preview_amd.system.lattice import Lattice
        for name in patch._LATTICE_METHODS:
            assert getattr(mods[root + ".system.lattice"].Lattice, name) is getattr(Lattice, name)
        patch.uninstall(handle)
        for ours, ref, name in patch.binding_table():
            assert getattr(mods[root + "." + ref], name) == ("placeholder", ref, name)
        # a renamed entry point on the reference side is an error, not a silent skip
        delattr(mods[root + ".routine.slater"], "get_emb_eri")
        with pytest.raises(AttributeError):
            patch.install(reference_package=root)
        h = patch.install(reference_package=root, strict=False, replace_hf=False)
        assert mods[root + ".routine.mfd"].HF == ("placeholder", "routine.mfd", "HF")
        patch.uninstall(h)
    finally:
        for k in list(mods):
            sys.modules.pop(k, None)


def _recorded_reference(root):
    """A module tree named like the reference's, holding a placeholder for every callable that golden G40 records
    (oracle/gen_golden.py gen_G40: names read off the reference's real module tree under the import shim)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G40_reference_names.json")) as f:
        rec = json.load(f)
    mods = {}

    def mk(name):
        if name not in mods:
            mods[name] = sys.modules[name] = types.ModuleType(name)
        return mods[name]
    mk(root)
    for ref, names in rec["modules"].items():
        parts = ref.split(".")
        for i in range(1, len(parts) + 1):
            mk(root + "." + ".".join(parts[:i]))
        for name in names:
            setattr(mods[root + "." + ref], name, ("placeholder", ref, name))
    mods[root + ".system.lattice"].Lattice = type("Lattice", (), {n: ("placeholder", n) for n in rec["Lattice"]})
    return rec, mods


def test_binding_table_matches_the_reference_tree():
    root = "recorded_libdmet_for_patch_test"
    rec, mods = _recorded_reference(root)
    try:
        for ours, ref, name in patch.binding_table():
            assert ref in rec["modules"] and name in rec["modules"][ref], (ref, name)
            assert hasattr(importlib.import_module(root + "." + ref), name), (ref, name)
        lat = importlib.import_module(root + ".system.lattice")
        for name in patch._LATTICE_METHODS:
            assert name in rec["Lattice"] and hasattr(lat.Lattice, name), name
        from libdmet_preview_amd.basis_transform import eri_transform as aet
        handle = patch.install(reference_package=root)
        try:
            rs = importlib.import_module(root + ".routine.slater")
            assert rs.get_emb_eri is aet.get_emb_eri
        finally:
            patch.uninstall(handle)
        rs = importlib.import_module(root + ".routine.slater")
        assert rs.get_emb_eri is not aet.get_emb_eri
    finally:
        for k in list(mods):
            sys.modules.pop(k, None)
