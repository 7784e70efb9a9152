"""Who asks the engine for the strip step 1 (eri_transform.strip_step1_wanted): host only."""


def test_strip_step1_request_rule(monkeypatch):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    for k in ("DMK_ERI_SPLIT1", "DMK_ERI_STRIP", "DMK_ERI_INV"):
        monkeypatch.delenv(k, raising=False)
    want = lambda *a: et.strip_step1_wanted(et.split_step1_wanted(*a))
    assert want(256, True, 224) and want(256, True, 192) and want(256, True, None)
    assert not want(256, True, 191)           # never a cache of the region: neither mode
    assert not want(256, False, 224)          # no token / no resident tensor
    assert not want(250, True, 224)           # the table path
    monkeypatch.setenv("DMK_ERI_INV", "0")
    assert want(256, True, 224)               # the uncached A/B run keeps the order
    monkeypatch.setenv("DMK_ERI_STRIP", "0")
    assert not want(256, True, 224) and et.split_step1_wanted(256, True, 224)      # K6l's order
    monkeypatch.delenv("DMK_ERI_STRIP")
    monkeypatch.setenv("DMK_ERI_SPLIT1", "0")
    assert not want(256, True, 224) and not et.split_step1_wanted(256, True, 224)  # both off
    assert not et.strip_step1_wanted(False)
