"""CPU: the plain-torch statements of instag_amd.metrics (frame figures, meter, dilated composition) and the C ABI of
csrc/metrics.hip."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instag_amd import metrics as M


def test_frame_metrics_torch_agrees_with_the_loss_functions(golden_dir):
    from instag_amd import losses
    g = np.load(f"{golden_dir}/g3_losses.npz")
    a, b = torch.from_numpy(g["a"]), torch.from_numpy(g["b"])
    rows = M.frame_metrics_torch(torch.stack([a, b]), torch.stack([b, a]), clamp=False)
    assert tuple(rows.shape) == (2, 5) and M.COLUMNS == ("l1", "mse", "psnr", "psnr_rgb", "ssim")
    for row, (x, y) in zip(rows, ((a, b), (b, a))):
        assert float(row[0]) == float(losses.l1_loss(x, y))
        assert float(row[1]) == float(((x - y) ** 2).mean())
        assert float(row[3]) == float(losses.psnr(x, y).mean())
        assert float(row[4]) == float(losses.ssim(x, y))
    # ... and with the reference's recorded values
    gp = float(g["psnr"].reshape(-1)[0])
    assert abs(float(rows[0, 0]) - float(g["l1"])) < 1e-7 and abs(float(rows[0, 4]) - float(g["ssim"])) < 1e-6
    assert abs(float(losses.psnr(a[None], b[None])) - gp) < 1e-4
    # metrics.py:127 on the same pair, as numpy computes it; the golden psnr is image_utils.psnr of the whole [1,3,H,W]
    # stack = the same figure
    want = -10 * np.log10(np.mean((g["a"] - g["b"]) ** 2))
    assert abs(float(rows[0, 2]) - float(want)) < 1e-5 and abs(float(rows[0, 2]) - gp) < 1e-4
    # the CPU path of the public function is the statement; the clamp only touches pred
    assert torch.equal(M.frame_metrics(torch.stack([a, b]), torch.stack([b, a]), clamp=False), rows)
    x = a * 1.4 - 0.2
    assert torch.equal(M.frame_metrics(x[None], (b * 1.4 - 0.2)[None]),
                       M.frame_metrics_torch(x.clamp(0, 1)[None], (b * 1.4 - 0.2)[None], clamp=False))
    same = M.frame_metrics_torch(a[None], a[None])
    assert float(same[0, 1]) == 0 and math.isinf(float(same[0, 2])) and float(same[0, 2]) > 0
    assert abs(float(same[0, 4]) - 1) < 1e-6


def test_quantisation_identities_hold_for_all_256_levels():
    k = np.arange(256)
    assert np.array_equal(np.float32(k) / np.float32(255), np.float32(k / 255.0))
    # every level is a fixed point: a frame read back and written again keeps its bytes
    lv = torch.arange(256, dtype=torch.float32) / 255.0
    assert torch.equal((lv * 255).to(torch.uint8), torch.arange(256, dtype=torch.uint8))
    assert torch.equal(M.quantize_frame(lv), lv)
    # torch's truncating cast == the reference's numpy line (synthesize_fuse.py:76) on values around every level
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.rand(100000, generator=g) * 1.2 - 0.1, lv, lv + 1e-7, lv - 1e-7,
                   torch.nextafter(lv, torch.tensor(2.0)), torch.nextafter(lv, torch.tensor(-1.0))])
    want = (x.clamp(0, 1).numpy() * 255).astype(np.uint8)
    assert np.array_equal((x.clamp(0, 1) * 255).to(torch.uint8).numpy(), want)
    # ... and what metrics.py:205-206 reads back from such a frame
    assert np.array_equal(M.quantize_frame(x).numpy(), torch.FloatTensor(want / 255.0).numpy())


def test_meter_averages_per_frame_values():
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(3, 3, 20, 24, generator=g)
    pred = gt + torch.tensor([0.01, 0.1, 0.3])[:, None, None, None] * torch.randn(3, 3, 20, 24, generator=g)
    meter = M.Meter("cpu")
    rows = M.frame_metrics(pred, gt, meter=meter)
    rep = meter.report()
    assert rep["frames"] == 3 and rep["lpips"] is None
    assert set(rep) == {"l1", "mse", "psnr", "psnr_rgb", "ssim", "lpips", "frames"}
    for i, k in enumerate(M.COLUMNS):
        assert abs(rep[k] - float(rows[:, i].double().mean())) < 1e-12
    # the reference's PSNRMeter (metrics.py:123-133): V += psnr of each frame, V / N -- not the PSNR of the mean MSE
    p, t = pred.clamp(0, 1).numpy(), gt.numpy()
    V = sum(-10 * np.log10(np.mean((p[i] - t[i]) ** 2)) for i in range(3))
    assert abs(rep["psnr"] - V / 3) < 1e-5
    assert abs(rep["psnr"] - (-10 * math.log10(rep["mse"]))) > 1.0
    # n_valid keeps a padded tail out; the LPIPS slot has its own count; clear() zeroes everything
    meter.clear()
    M.frame_metrics(pred, gt, meter=meter, n_valid=2)
    meter.add_lpips(torch.tensor([0.25, 0.75, 0.5]))
    rep = meter.report()
    assert rep["frames"] == 2 and abs(rep["l1"] - float(rows[:2, 0].double().mean())) < 1e-12 and rep["lpips"] == 0.5
    meter.clear()
    assert meter.report()["frames"] == 0 and not meter.state.any()
    with pytest.raises(ValueError):
        M.frame_metrics(pred, gt, n_valid=4)


def _synthesize_fuse_lines(face, alpha, mouth, alpha_mouth, scene, dilate):
    """synthesize_fuse.py:29-32, 65-76."""
    def dilate_fn(bin_img, ksize=13):
        pad = (ksize - 1) // 2
        return F.max_pool2d(bin_img, kernel_size=ksize, stride=1, padding=pad)
    if dilate:
        alpha_mouth = dilate_fn(alpha_mouth[None])[0]
    mouth_image = mouth + scene * (1.0 - alpha_mouth)
    image = face + mouth_image * (1.0 - alpha)
    return (image[0:3, ...].clamp(0, 1).permute(1, 2, 0).detach().cpu().numpy() * 255).astype(np.uint8)


@pytest.mark.parametrize("dilate", [False, True])
def test_dilated_composition_statement_is_the_reference_lines(dilate):
    g = torch.Generator().manual_seed(2)
    H, W = 37, 53
    alpha, alpha_mouth = torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g) ** 4
    face, mouth = torch.rand(3, H, W, generator=g) * alpha, torch.rand(3, H, W, generator=g) * alpha_mouth
    scene = torch.rand(3, H, W, generator=g)
    want = _synthesize_fuse_lines(face, alpha, mouth, alpha_mouth, scene, dilate)
    image, u8 = M.infer_compose_torch(face, alpha, mouth, alpha_mouth, torch.zeros(3), scene, 13 if dilate else 1)
    assert np.array_equal(u8.numpy(), want) and tuple(u8.shape) == (H, W, 3)
    assert float(image.min()) >= 0 and float(image.max()) <= 1
    # the public function's CPU path is the statement; dilation changes the frame
    image2, u82 = M.infer_compose(face, alpha, mouth, alpha_mouth, torch.zeros(3), scene, 13 if dilate else 1, True)
    assert torch.equal(image, image2) and torch.equal(u8, u82)
    if dilate:
        assert not np.array_equal(want, _synthesize_fuse_lines(face, alpha, mouth, alpha_mouth, scene, False))
    for bad in (0, 2, 33):
        with pytest.raises(ValueError):
            M.infer_compose(face, alpha, mouth, alpha_mouth, torch.zeros(3), scene, bad)


def test_frame_lpips_on_the_cpu_is_the_package_call_with_normalize():
    from instag_amd import lpips as LP
    w = LP.LPIPSWeights.random(0)
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(2, 3, 64, 48, generator=g)
    pred = (gt + 0.05 * torch.randn(2, 3, 64, 48, generator=g)).clamp(0, 1)
    meter = M.Meter("cpu")
    got = M.FrameLPIPS(w, 64, 48)(pred, gt, meter=meter)
    want = LP.lpips_torch(2 * gt - 1, 2 * pred - 1, w).reshape(-1)          # lpips(truth, pred, normalize=True)
    assert torch.equal(got, want) and abs(meter.report()["lpips"] - float(want.double().mean())) < 1e-12


def test_new_symbols_are_exported_and_validate_their_arguments():
    from instag_amd import _lib
    names = ("instag_frame_metrics_num_partials", "instag_frame_metrics", "instag_meter_add", "instag_infer_compose")
    lib = _lib.lib()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.instag_abi_version() == 10
    assert lib.instag_frame_metrics_num_partials(3, 37, 53) == 3 * 9 * 3 * 4
    assert lib.instag_frame_metrics_num_partials(1, 16, 16) == 9 and lib.instag_frame_metrics_num_partials(0, 4, 4) == 0
    one = ctypes.c_void_p(16)
    assert lib.instag_frame_metrics(None, one, 1, 8, 8, 0, one, one, None, 1, None) != 0
    assert b"NULL" in lib.instag_last_error()
    assert lib.instag_frame_metrics(one, one, 1, 8, 8, 4, one, one, None, 1, None) != 0
    assert b"flag" in lib.instag_last_error()
    assert lib.instag_frame_metrics(one, one, 2, 8, 8, 3, one, one, None, 3, None) != 0
    assert b"n_valid" in lib.instag_last_error()
    for bad in (0, 2, 33):
        assert lib.instag_infer_compose(one, one, one, one, one, None, bad, one, None, 8, 8, None) != 0
        assert b"dilate" in lib.instag_last_error()
    assert lib.instag_infer_compose(one, one, one, one, None, None, 1, one, None, 8, 8, None) != 0
    assert b"NULL" in lib.instag_last_error()
    assert lib.instag_meter_add(None, 1, one, None) != 0 and b"NULL" in lib.instag_last_error()
