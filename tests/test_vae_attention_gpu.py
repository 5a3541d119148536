"""fluxmi_vae_attention (csrc/vae_attention.hip) on the GPU: the kernel against the fp64 reference under the gate of tests/vae_attention_ref.py
at every size where it takes another path, its bits (run to run, a sample alone against the sample in a batch), a size past the [P, P]
matrix's 32-bit limit, and the whole autoencoder with attention="streaming" under the gates the default path is held to."""
import os

import pytest
import torch

import vae_attention_ref as var
from helper_refs import bits, poison, sentinel_like

pytestmark = pytest.mark.gpu

QR = 64  # query rows per workgroup (csrc/vae_attention.hip)
# 1: one key; 63 / 64 / 65: the edges of one tile and one workgroup; 200, 1089: ragged last tile, several workgroups;
# 385 = 4 * QR + 2 * KEY_TILE + 1: two key tiles past a multiple of the workgroup's rows, plus one
PS = [1, 63, 64, 65, 200, 1089, 4 * QR + 2 * var.KEY_TILE + 1]
DS = [64, 512]


def run_kernel(ops, dev, q, k, v, bias, P, pad_cols=8):
    """q, k, v [B, P, D] on the host -> (out [B, P, D], frame ok): q / k as column windows of one wider buffer (ld_qk = 2 D + 16), V^T with
    ld_vt > Pp, every pad poisoned with +-1e4, `out` a window of a sentinel-filled buffer"""
    B, _, D = q.shape
    Pp = -(-P // 64) * 64
    qk = torch.zeros(B, Pp, 2 * D + 16, dtype=torch.bfloat16)
    qk[:, :P, :D], qk[:, :P, D + 8 : 2 * D + 8] = q, k
    qk = poison(qk, P, 1)
    vt = torch.zeros(B, D, Pp + pad_cols, dtype=torch.bfloat16)
    vt[:, :, :P] = v.transpose(1, 2)
    vt = poison(vt, P, 2)
    qk, vt = qk.to(dev), vt.to(dev)
    buf = sentinel_like((B, Pp + 1, D + 16), dev)
    out = buf[:, :Pp, 8 : 8 + D]
    got = ops.vae_attention(qk[:, :, :D], qk[:, :, D + 8 : 2 * D + 8], vt[:, :, :Pp], P, v_bias=bias.to(dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    res = buf.cpu()
    frame = res.clone()
    frame[:, :P, 8 : 8 + D] = sentinel_like((B, P, D))
    return res[:, :P, 8 : 8 + D].contiguous(), bool((bits(frame) == bits(sentinel_like(frame.shape))).all())


@pytest.fixture(scope="module")
def ops():
    from fluxmi import ops as o

    return o


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_kernel_against_the_gate(ops, dev, P, D):
    for B in (1, 3):
        for fam in var.FAMILIES:
            q, k, v, b = var.inputs(fam, B, P, D, seed=3)
            got, frame_ok = run_kernel(ops, dev, q, k, v, b, P)
            var.assert_close(got, var.gate(q, k, v, b), f"vae_attention {fam} D={D} P={P} B={B}")
            assert frame_ok, f"{fam} D={D} P={P} B={B}: a row >= P or the frame around `out` was written"


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", [65, 1089])
def test_bits_run_to_run_and_sample_alone(ops, dev, P, D):
    q, k, v, b = var.inputs("randn", 3, P, D, seed=4)
    a, _ = run_kernel(ops, dev, q, k, v, b, P)
    a2, _ = run_kernel(ops, dev, q, k, v, b, P)
    assert torch.equal(bits(a), bits(a2)), "two runs differ"
    for i in range(3):
        alone, _ = run_kernel(ops, dev, q[i : i + 1], k[i : i + 1], v[i : i + 1], b, P)
        assert torch.equal(bits(alone[0]), bits(a[i])), f"sample {i} alone differs from the same sample inside B = 3"


def test_past_the_score_matrix_limit(ops, dev):
    """P = 46400 > 46340: a [P, P] bf16 matrix would pass 4 GiB.  Three blocks of 64 query rows against fp64 computed for those rows only."""
    P, D = 46400, 512
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, P, D, generator=g).bfloat16() for _ in range(3))
    b = torch.randn(D, generator=g).bfloat16()
    qk = torch.cat((q, k), 2).to(dev)
    vt = v.transpose(1, 2).contiguous().to(dev)
    got = ops.vae_attention(qk[:, :, :D], qk[:, :, D:], vt, P, v_bias=b.to(dev)).cpu()
    rows = torch.cat([torch.arange(r0, r0 + 64) for r0 in (0, (P // 2) // 64 * 64, P - 64)])
    var.assert_close(got[:, rows], var.gate(q[:, rows], k, v, b), f"vae_attention randn D={D} P={P}, rows 0.., {int(rows[64])}.., {P - 64}..")


def test_op_refuses_bad_shapes(ops, dev):
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="share shape and strides"):
        ops.vae_attention(z(1, 64, 64), z(1, 64, 128)[:, :, :64], z(1, 64, 64), 64)
    with pytest.raises(ValueError, match="D=128"):
        ops.vae_attention(z(1, 64, 128), z(1, 64, 128), z(1, 128, 64), 64)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.vae_attention(z(1, 72, 64), z(1, 72, 64), z(1, 64, 72), 70)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.vae_attention(z(1, 64, 64), z(1, 64, 64), z(1, 64, 64), 65)
    with pytest.raises(ValueError, match="vt must be"):
        ops.vae_attention(z(1, 128, 64), z(1, 128, 64), z(1, 64, 64), 100)
    with pytest.raises(ValueError, match="out must be"):
        ops.vae_attention(z(1, 128, 64), z(1, 128, 64), z(1, 64, 128), 100, out=z(1, 99, 64))
    with pytest.raises(ValueError, match="v_bias"):
        ops.vae_attention(z(1, 128, 64), z(1, 128, 64), z(1, 64, 128), 100, v_bias=z(32))


# ---- the whole autoencoder ------------------------------------------------------------------------------------------------------------------
rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G8 = dict(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2], num_res_blocks=1, z_channels=4, scale_factor=0.3611, shift_factor=0.1159)


def g8_autoencoder(dev):
    from safetensors.torch import load_file

    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    g = load_file(os.path.join(GOLDEN, "g8_vae.safetensors"))
    ae = AutoEncoder(AutoEncoderParams(**G8))
    ae.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return ae.to(dev), g


def test_small_vae_streaming_matches_reference_fixture(dev):
    """the gates of test_engine_gpu.py's g8 decoder / encoder tests, with attention="streaming" (mid width 64)"""
    ae, g = g8_autoencoder(dev)
    z, x = g["z"].to(dev), g["enc_x"].to(dev)
    out_g, mom_g = ae.decode(z).float().cpu(), ae.encode_moments(x).float().cpu()
    ae.attention = "streaming"
    out, mom = ae.decode(z).float().cpu(), ae.encode_moments(x).float().cpu()
    assert out.shape == g["ref_fp32"].shape and torch.isfinite(out).all()
    e_native, e_ref = rel(out, g["ref_fp32"]), rel(g["ref_autocast"], g["ref_fp32"])
    print(f"VAE decode (streaming): native vs fp32 reference {e_native:.3e}; reference autocast vs fp32 {e_ref:.3e}; native vs oracle-autocast "
          f"{rel(out, g['oracle_autocast']):.3e}; streaming vs gemm {rel(out, out_g):.3e}")
    assert e_native <= 1.5 * e_ref
    assert rel(out, g["oracle_autocast"]) <= 1.5e-2
    assert mom.shape == g["enc_moments_fp32"].shape and torch.isfinite(mom).all()
    m_native, m_ref = rel(mom, g["enc_moments_fp32"]), rel(g["enc_moments_autocast"], g["enc_moments_fp32"])
    print(f"VAE encode (streaming): native vs fp32 reference {m_native:.3e}; reference autocast vs fp32 {m_ref:.3e}; native vs oracle-autocast "
          f"{rel(mom, g['enc_oracle_moments_autocast']):.3e}; streaming vs gemm {rel(mom, mom_g):.3e}")
    assert m_native <= 1.5 * m_ref
    assert rel(mom, g["enc_oracle_moments_autocast"]) <= 2e-2
    # a batch goes through ONE attention launch
    two = ae.decode(torch.cat((z, z.flip(-1)), 0)).float().cpu()
    n = z.shape[0]
    assert two.shape[0] == 2 * n and torch.isfinite(two).all() and rel(two[:n], out) <= 1e-2


def test_full_size_vae_streaming_matches_reference_fixture(dev):
    """the gate of test_engine_gpu.py's full-geometry test (mid width 512, 256 x 256 image), with attention="streaming" """
    from safetensors.torch import load_file

    import vae_oracle as vo
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    g = load_file(os.path.join(GOLDEN, "g11_vae_full.safetensors"))
    ae = AutoEncoder(AutoEncoderParams(**vo.FULL_PARAMS))
    ae.load_state_dict(vo.synth_state_dict({k: v.shape for k, v in ae.state_dict().items()}, seed=7), strict=True)
    ae.to(dev)
    z, x = vo.full_inputs()
    out_g, mom_g = ae.decode(z.to(dev)).float().cpu(), ae.encode_moments(x.to(dev)).float().cpu()
    ae.attention = "streaming"
    out = ae.decode(z.to(dev)).float().cpu()
    assert out.shape == g["dec_ref_fp32"].shape and torch.isfinite(out).all()
    e_nat, e_ref = rel(out, g["dec_ref_fp32"]), rel(g["dec_ref_autocast"], g["dec_ref_fp32"])
    mom = ae.encode_moments(x.to(dev)).float().cpu()
    assert mom.shape == g["enc_moments_fp32"].shape and torch.isfinite(mom).all()
    m_nat, m_ref = rel(mom, g["enc_moments_fp32"]), rel(g["enc_moments_autocast"], g["enc_moments_fp32"])
    print(f"full-size VAE (streaming): decode native vs fp32 reference {e_nat:.3e} (reference autocast {e_ref:.3e}; streaming vs gemm "
          f"{rel(out, out_g):.3e}); encode moments {m_nat:.3e} (reference autocast {m_ref:.3e}; streaming vs gemm {rel(mom, mom_g):.3e})")
    assert e_nat <= 1.5 * e_ref and m_nat <= 1.5 * m_ref


def test_streaming_at_a_pixel_count_off_the_8_grid(dev):
    """test_kontext_gpu.py's off-grid case (a 6 x 10 latent: 60 pixels, padded to 64 keys) through the streaming path, under that test's bound"""
    import vae_oracle as vo
    from modules.autoencoder import AutoEncoder, AutoEncoderParams

    params = dict(resolution=32, in_channels=3, ch=32, out_ch=3, ch_mult=[1, 2, 2, 2], num_res_blocks=1, z_channels=16, scale_factor=0.3611,
                  shift_factor=0.1159)
    torch.manual_seed(0)
    ae = AutoEncoder(AutoEncoderParams(**params))
    sd = {k: v.clone() for k, v in ae.state_dict().items()}
    ae.to(dev)
    ae.attention = "streaming"
    x = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(2)) * 2 - 1
    mom = ae.encode_moments(x.to(dev)).float().cpu()
    ref = vo.encode_moments(sd, params, x, autocast=True).float()
    assert mom.shape == ref.shape == (1, 32, 6, 10) and torch.isfinite(mom).all()
    e = rel(mom, ref)
    print(f"VAE encode at a 6 x 10 latent (streaming): native vs oracle-autocast rel-L2 {e:.3e}")
    assert e <= 2e-2


def test_default_path_is_untouched(dev, monkeypatch):
    """attention="gemm" never reaches the new op and still runs the row softmax"""
    from fluxmi import ops as o

    ae, g = g8_autoencoder(dev)
    assert ae.attention == "gemm"
    calls = []
    real = o.softmax_rows

    def boom(*a, **k):
        raise AssertionError("the default path called ops.vae_attention")

    monkeypatch.setattr(o, "vae_attention", boom)
    monkeypatch.setattr(o, "softmax_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ae.decode(g["z"].to(dev))
    ae.encode_moments(g["enc_x"].to(dev))
    assert len(calls) == g["z"].shape[0] + g["enc_x"].shape[0]  # one row softmax per image
