"""Host-side checks of the MXFP8 GEMM and encoder-layer entry points (no GPU needed)."""
import ctypes

import pytest

BASE = [(5672, 2304, 768), (5672, 768, 768), (5672, 3072, 768), (5672, 768, 3072)]
LARGE = [(2442, 3072, 1024), (2442, 1024, 1024), (2442, 4096, 1024), (2442, 1024, 4096)]


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return ctypes.CDLL(hip.LIB_PATH)


def test_mxfp8_encoder_symbols_are_declared_and_exported(lib):
    from peneo_amd import hip
    for name in ("peneo_mxfp8_quantize_rows_bf16", "peneo_gemm_mxfp8_supported", "peneo_gemm_mxfp8", "peneo_layernorm_mxfp8_supported",
                 "peneo_layernorm_fwd_mxfp8", "peneo_encoder_layer_mxfp8_supported", "peneo_encoder_layer_fwd_mxfp8"):
        assert name in hip.SIGNATURES
        assert hasattr(lib, name)
    assert lib.peneo_version() >= 102


@pytest.mark.parametrize("M,N,K", BASE + LARGE)
def test_support_query_accepts_the_model_shapes(lib, M, N, K):
    assert lib.peneo_gemm_mxfp8_supported(M, N, K) == 1


@pytest.mark.parametrize("M,N,K", [(1, 32, 128), (7, 96, 384), (100000, 32, 4096)])
def test_support_query_accepts_any_m_with_n_32_and_k_128(lib, M, N, K):
    assert lib.peneo_gemm_mxfp8_supported(M, N, K) == 1


@pytest.mark.parametrize("M,N,K", [(64, 64, 100), (64, 64, 144), (64, 48, 128), (64, 100, 768), (0, 64, 128), (64, 0, 128), (64, 64, 0),
                                   (-5, 64, 128), (64, -32, 128), (64, 64, -128)])
def test_support_query_refuses_what_the_kernel_cannot_hold(lib, M, N, K):
    # K % 32 != 0; N % 32 != 0 (an MX output block is 32 consecutive n, and the kernel's tiles are whole blocks); non-positive sizes
    assert lib.peneo_gemm_mxfp8_supported(M, N, K) == 0


def test_layer_support_query(lib):
    assert lib.peneo_encoder_layer_mxfp8_supported(5672, 768, 3072) == 1
    assert lib.peneo_encoder_layer_mxfp8_supported(2442, 1024, 4096) == 1
    assert lib.peneo_encoder_layer_mxfp8_supported(4096, 192, 768) == 0      # K = 192 is not a whole number of 128-deep stages
    assert lib.peneo_encoder_layer_mxfp8_supported(0, 768, 3072) == 0


def test_struct_size_is_reported(lib):
    from peneo_amd import hip
    lib.peneo_struct_bytes.restype = ctypes.c_size_t
    assert lib.peneo_struct_bytes(3) == ctypes.sizeof(hip.EncoderLayerMxfp8) == 18 * ctypes.sizeof(ctypes.c_void_p) + 8


def test_fused_layernorm_support_query(lib):
    assert [lib.peneo_layernorm_mxfp8_supported(h) for h in (768, 1024, 256, 192, 1280, 0, -256)] == [1, 1, 1, 0, 0, 0, 0]


def _tiny(name, backbone_cfg):
    from seeded import peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    pcfg = peneo_config(name, backbone_cfg)
    return PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))


def test_model_switch_refusals_need_no_gpu():
    import torch
    from seeded import layoutlmv3_config, lilt_config
    m = _tiny("layoutlmv3-base", dict(layoutlmv3_config("base"), num_hidden_layers=1))
    with pytest.raises(ValueError):
        m.set_encoder_format("mxfp8")            # fp32 compute dtype
    m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError):
        m.set_encoder_format("fp8")
    assert m.set_encoder_format("mxfp8") is m and m.backbone.encoder_format == "mxfp8"
    assert m.set_encoder_format("bf16") is m and m.backbone.encoder_format == "bf16"
    narrow = _tiny("layoutlmv3-base", layoutlmv3_config("tiny")).set_compute_dtype(torch.bfloat16)
    if narrow.backbone.config.hidden_size % 128 != 0:
        with pytest.raises(ValueError):
            narrow.set_encoder_format("mxfp8")   # a width peneo_gemm_mxfp8 does not hold
    lilt = _tiny("lilt-roberta-en-base", dict(lilt_config("base"), num_hidden_layers=1)).set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError, match="LiLT"):
        lilt.set_encoder_format("mxfp8")
