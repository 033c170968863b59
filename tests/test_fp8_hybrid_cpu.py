"""mixer_weights (fp8 Mamba2 projections of the hybrid) on the CPU: the argument is checked before any GPU work, by
make_engine, HybridEngine and Zonos alike, and `weights` keeps meaning the MLP projections."""
import pytest

from zonos_vibes_amd.config import hybrid_config, tiny_hybrid, tiny_transformer


def test_mixer_weights_argument_validation():
    from zonos_vibes_amd.engine import WEIGHT_FORMATS, check_mixer_weights, has_mamba2_mixers, make_engine
    from zonos_vibes_amd.hybrid import HybridEngine
    from zonos_vibes_amd.model import Zonos
    assert WEIGHT_FORMATS == ("bf16", "fp8")
    assert has_mamba2_mixers(tiny_hybrid()) and not has_mamba2_mixers(tiny_transformer(2))
    assert not has_mamba2_mixers(hybrid_config(512, 2, [0, 1], 4, 1))       # a hybrid config of MHA layers only
    for cfg in (tiny_hybrid(), tiny_transformer(2)):
        check_mixer_weights("bf16", cfg)                                     # accepted on both backbones
        for make in (make_engine, Zonos):
            with pytest.raises(ValueError, match="int8"):
                make(cfg, "cpu", mixer_weights="int8")
    with pytest.raises(ValueError, match="int8"):
        HybridEngine(tiny_hybrid(), "cpu", mixer_weights="int8")
    check_mixer_weights("fp8", tiny_hybrid())
    for make in (make_engine, Zonos, HybridEngine):
        with pytest.raises(NotImplementedError, match="mixer_weights"):
            make(tiny_transformer(2), "cpu", mixer_weights="fp8")
    with pytest.raises(NotImplementedError, match="mixer_weights"):
        make_engine(hybrid_config(512, 2, [0, 1], 4, 1), "cpu", mixer_weights="fp8")


def test_weights_fp8_still_refuses_the_hybrid():
    """`weights` is the MLP projections' format: on the hybrid it raises as before, whatever mixer_weights says."""
    from zonos_vibes_amd.engine import make_engine
    from zonos_vibes_amd.model import Zonos
    for make in (make_engine, Zonos):
        for mw in ("bf16", "fp8"):
            with pytest.raises(NotImplementedError, match="weights"):
                make(tiny_hybrid(), "cpu", weights="fp8", mixer_weights=mw)


def test_binding_declares_the_expansion_entry_point():
    from zonos_vibes_amd import _lib
    assert "zmi_unpack_fp8" in _lib.EXPORTED
    assert len(_lib._SIGS["zmi_unpack_fp8"][1]) == 6
