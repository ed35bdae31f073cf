"""CPU: the plain-torch statements of instag_amd.frame_store (ingest, unpack, a store on the CPU device) against the
reference's numpy lines, and the C ABI of csrc/frames.hip."""
import ctypes

import numpy as np
import pytest
import torch

from instag_amd import frame_store as FS
from tests import frame_store_helpers as H


def test_ingest_torch_composite_is_the_numpy_expression_on_all_triples():
    """All 256^3 (torso, alpha, bc) triples, each in every channel, in sixteen slabs of 256 rows."""
    seen = 0
    for r in range(0, 4096, 256):
        torso, bc = H.triples(slice(r, r + 256))
        want = H.composite_numpy(torso, bc)
        n = torso.shape[0]
        z1 = torch.zeros(1, n, 4096, dtype=torch.uint8)
        _, bg, _, _ = FS.ingest_torch(z1[..., None].expand(1, n, 4096, 3), torch.from_numpy(torso)[None],
                                      torch.from_numpy(bc), z1[..., None].expand(1, n, 4096, 3), z1)
        assert np.array_equal(bg[0].numpy(), want)
        seen += n * 4096
    assert seen == 256 ** 3
    # the expression is not the integer form: the statement must not be "simplified"
    torso, bc = H.triples(slice(2048, 2304))
    t, a, b = torso[..., 0].astype(np.int64), torso[..., 3].astype(np.int64), bc[..., 0].astype(np.int64)
    assert int((H.composite_numpy(torso, bc)[..., 0] != (t * a + b * (255 - a)) // 255).sum()) > 0


@pytest.mark.parametrize("shape", H.SHAPES)
def test_ingest_torch_masks_are_the_reference_lines(shape):
    raw = H.raw_frames(3, *shape, seed=7)
    rgb, bg, mask, counts = FS.ingest_torch(*(torch.from_numpy(raw[k]) for k in ("gt", "torso", "bc", "parsing", "teeth")))
    face, hair, mouth = H.masks_numpy(raw["parsing"], raw["teeth"])
    m = mask.numpy()
    assert np.array_equal(m & 1, face) and np.array_equal((m >> 1) & 1, hair) and np.array_equal((m >> 2) & 1, mouth)
    assert np.array_equal(rgb.numpy(), raw["gt"])
    assert np.array_equal(bg.numpy(), H.composite_numpy(raw["torso"], raw["bc"][None]))
    want = np.stack([x.reshape(3, -1).sum(1) for x in (face, hair, mouth)], axis=1)
    assert np.array_equal(counts.numpy(), want) and counts.dtype == torch.int32
    assert int(counts[1, 2]) == 0 and int(counts[0, 2]) > 0            # one frame without a mouth
    # every rule and every near miss is present: teeth flip face pixels off and non-face pixels on
    t = raw["teeth"].astype(bool)
    blue = (raw["parsing"] == np.array([0, 0, 255], dtype=np.uint8)).all(-1)
    assert (blue & t).any() and not face[blue & t].any() and face[~blue & t].all()
    for near in ((0, 0, 254), (100, 100, 99), (0, 0, 1), (1, 0, 255)):
        sel = (raw["parsing"] == np.array(near, dtype=np.uint8)).all(-1) & ~t
        assert sel.any() and not (face[sel].any() or hair[sel].any() or mouth[sel].any())


@pytest.mark.parametrize("C,L", [(29, 16), (1, 512)])
def test_audio_window_is_get_audio_features_mode_2(C, L):
    from instag_amd.ave_encoder import frame_window
    T = 12
    table = H.audio_table(T, C, L, 3)
    for idx in (0, 1, 3, 4, T - 4, T - 3, T - 1, T):
        w = FS.audio_window(table, idx)
        assert tuple(w.shape) == (8, C, L)
        for r in range(8):
            src = idx - 4 + r
            assert torch.equal(w[r], table[src] if 0 <= src < T else torch.zeros(C, L))
        if C == 1:
            assert torch.equal(w, frame_window(table.permute(0, 2, 1), idx))


@pytest.mark.parametrize("priors", [False, True])
def test_cpu_store_unpacks_into_packed_frames_and_keeps_the_padding(priors):
    from instag_amd.train import make_frame, Frame
    F, (Hh, W), T = 3, (5, 7), 12
    store, raw = H.build_store("cpu", F, Hh, W, 11, [0, 5, T - 1], H.audio_table(T, 29, 16, 1), priors=priors)
    assert len(store) == F and store.nbytes > F * FS.store_stride(Hh, W)
    face, hair, mouth = H.masks_numpy(raw["parsing"], raw["teeth"])
    assert np.array_equal(store.counts.numpy()[:, 2], mouth.reshape(F, -1).sum(1))
    for i in range(F):
        want = store.unpack_torch(i)
        assert torch.equal(want["original_image"], torch.from_numpy(raw["gt"][i]).permute(2, 0, 1) / 255.0)
        assert np.array_equal(want["face_mask"].numpy(), face[i]) and want["face_mask"].dtype == torch.bool
        assert torch.equal(want["lips_rect"], raw["lips_rect"][i]) and torch.equal(want["au_exp"], raw["au_exp"][i])
        assert torch.equal(want["world_view_transform"], raw["cameras"][i].world_view_transform)
        f = store.frame(i)
        assert set(k for k, _, _ in f._layout) == set(want) and (f.FoVx, f.image_height) == (store.FoVx, Hh)
        # the same layout as a frame packed by make_frame from the statement
        cam = raw["cameras"][i]
        g = make_frame(cam, dict(want, gt_image=want["original_image"])).packed()
        assert g._layout == f._layout and torch.equal(g._buf, f._buf)
        # copy_from with a handle writes the tensors only
        static = f.packed()
        static._buf.fill_(0xA5)
        static.copy_from(store.ref((i + 1) % F))
        other = store.frame((i + 1) % F)
        written = torch.zeros_like(static._buf, dtype=torch.bool)
        offs, _ = FS._offsets(static._layout)
        for (k, s, d), o in zip(static._layout, offs):
            written[o:o + FS._nbytes(s, d)] = True
        assert torch.equal(static._buf[written], other._buf[written]) and bool((static._buf[~written] == 0xA5).all())
    # a handle behaves as the frame it stands for
    h = store.ref(1, background=False)
    assert "background" not in h.talking_dict and torch.equal(h.original_image, store.frame(1).original_image)
    assert isinstance(h.clone_static(), Frame)
    with pytest.raises(IndexError):
        store.ref(F)
    if not priors:
        with pytest.raises(ValueError):
            store.unpack_into(store.empty_frame(priors=True), 0)


def test_new_symbols_are_exported_and_validate_their_arguments():
    from instag_amd import _lib
    lib = _lib.lib()
    for n in ("instag_frame_store_stride", "instag_frame_record_dwords", "instag_frame_ingest", "instag_frame_unpack"):
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.instag_abi_version() == 10
    for hw in H.SHAPES + ((512, 512),):
        assert lib.instag_frame_store_stride(*hw) == FS.store_stride(*hw)
    assert lib.instag_frame_store_stride(0, 4) == 0 and lib.instag_frame_record_dwords() == FS.REC_DWORDS
    one, E_ARG = ctypes.c_void_p(256), 1

    def ingest(gt=one, F=1, Hh=4, W=4, store=one):
        return lib.instag_frame_ingest(gt, one, one, one, one, F, Hh, W, store, one, None)

    assert ingest(gt=None) == E_ARG and b"NULL" in lib.instag_last_error()
    assert ingest(Hh=0) == E_ARG and b"image size" in lib.instag_last_error()
    assert ingest(F=0) == E_ARG and b"frames" in lib.instag_last_error()
    assert ingest(gt=ctypes.c_void_p(258)) == E_ARG and b"aligned" in lib.instag_last_error()
    assert ingest(store=ctypes.c_void_p(260)) == E_ARG and b"aligned" in lib.instag_last_error()

    def unpack(**kw):
        a = _lib.FrameUnpackArgs()
        for k in ("store", "records", "audio", "dst"):
            setattr(a, k, 256)
        a.F, a.H, a.W, a.idx, a.audio_index, a.T, a.audio_row = 3, 5, 7, 2, 0, 12, 464
        offs, total = FS._offsets(tuple((k, s, d) for k, s, d in _layout(5, 7)))
        for (k, _, _), o in zip(_layout(5, 7), offs):
            setattr(a, FS._ARG_OF[k], o)
        a.off_background = a.off_normal = a.off_depth = -1
        a.dst_bytes = total
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.instag_frame_unpack(ctypes.byref(a), None)

    def _layout(Hh, W):
        s = FS.FrameStore("cpu")
        s.H, s.W = Hh, W
        return s.layout()

    assert lib.instag_frame_unpack(None, None) == E_ARG and b"NULL" in lib.instag_last_error()
    for k in ("store", "records", "audio", "dst"):
        assert unpack(**{k: None}) == E_ARG and b"NULL" in lib.instag_last_error()
    for idx in (-1, 3):
        assert unpack(idx=idx) == E_ARG and b"idx" in lib.instag_last_error()
    for ai in (-1, 13):
        assert unpack(audio_index=ai) == E_ARG and b"audio index" in lib.instag_last_error()
    assert unpack(H=0) == E_ARG and b"image size" in lib.instag_last_error()
    assert unpack(W=-3) == E_ARG and b"image size" in lib.instag_last_error()
    # bad layouts: a tensor past the end of the buffer, a missing one, a misaligned one, priors the store lacks
    assert unpack(dst_bytes=100) == E_ARG and b"does not fit" in lib.instag_last_error()
    assert unpack(off_auds=-1) == E_ARG and b"does not fit" in lib.instag_last_error()
    assert unpack(off_face=2) == E_ARG and b"does not fit" in lib.instag_last_error()
    assert unpack(off_normal=0, off_depth=512) == E_ARG and b"priors" in lib.instag_last_error()
    assert unpack(off_normal=0, normal=256, depth=256) == E_ARG and b"priors" in lib.instag_last_error()
