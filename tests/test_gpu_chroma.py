"""The chromatic-aberration remap on the GPU (``chromatic=``, csrc/kernels_chroma.hip) against the CPU oracle.

The contract: channel ``c`` of the result is, byte for byte, channel ``c`` of what the plain entry point gives for
``transformer * PolynomialScaler(coefs_c)``.  The plain path is byte-exact against the oracle, so the expected image is composed from
``oracle.get_map`` / ``oracle.remap`` of the three channel specs -- no restatement, no tolerance.  Sources are uniform noise, so that a
channel shifted by a few hundredths of a pixel changes bytes; every case first asserts that the expected image differs from the
UNCORRECTED oracle image in at least 5 % of its pixels: a condition on the inputs, so that no case passes with the feature ignored.

(The engine has one kernel family for this, ``chroma``: it samples from global memory.  The LDS-staged bilinear form the issue describes
is not part of the change, so the three inputs of its case 8 are held to that family.)"""
import numpy as np
import pytest
import torch

import chainspecs as CS
from test_oracle_golden import assert_maps_match

pytestmark = pytest.mark.gpu

RED = [0, 1.004, 0, -0.006]
BLUE = [0, 0.997, 0, 0.005]
COEFS = {"b": BLUE, "g": None, "r": RED}
BORDER_VALUE = (7, 130, 250)
EQUI_SPEC = [("equirect_enc", True), CS.EQUI]


@pytest.fixture(scope="module")
def V():
    import vr180_convert_amd as V

    return V


@pytest.fixture(scope="module")
def R():
    from vr180_convert_amd import remapper

    return remapper


@pytest.fixture(scope="module")
def CA():
    from vr180_convert_amd import chromatic

    return chromatic


@pytest.fixture(scope="module")
def ca(CA):
    return CA.ChromaticAberration(red=RED, blue=BLUE)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pattern(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 7 + yy * 3) % 251, (xx * 5 + yy * 11 + 40) % 253, (xx * 13 + yy * 2 + 90) % 255], axis=-1).astype(np.uint8)


_MAPS: dict = {}


def channel_specs(spec, coefs=COEFS):
    return [spec + [("poly", coefs[c])] if coefs[c] is not None else spec for c in "bgr"]


def oracle_map(O, spec, radius, size_input, size_output):
    key = (repr(spec), float(radius), tuple(size_input), tuple(size_output))
    if key not in _MAPS:
        _MAPS[key] = O.get_map(spec, radius=radius, size_input=size_input, size_output=size_output)
    return _MAPS[key]


def expect(O, spec, img, *, size_output, radius, interp, border=0, bval=0, dst=None, coefs=COEFS, min_changed=0.05):
    """(expected, uncorrected): the per-channel oracle composition and the plain oracle image; asserts that they differ enough"""
    size_in = img.shape[:2]

    def one(s):
        xm, ym = oracle_map(O, s, radius, size_in, size_output)
        return O.remap(img, xm, ym, interp, border, bval, dst=None if dst is None else dst.copy())

    plain = one(spec)
    want = np.stack([one(s)[..., c] for c, s in enumerate(channel_specs(spec, coefs))], axis=-1)
    changed = float((want != plain).any(axis=2).mean())
    assert changed >= min_changed, f"the inputs do not tell the correction apart: {changed:.3f} of the pixels differ"
    return want, plain


def families(kinds):
    """the kernel family per launch group, whether or not a fix-up pass followed (where that is not what the case is about)"""
    return [k.split("+")[0] for k in kinds]


def up(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. interpolation x border grid
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
def test_interpolation_and_border_grid(V, R, ca, oracle_mod, interp, border):
    img = noise(61, 83, 1)
    fill = pattern(70, 90)
    want, _ = expect(oracle_mod, EQUI_SPEC, img, size_output=(90, 70), radius=30.0, interp=interp, border=border, bval=BORDER_VALUE, dst=fill)
    dst = up(fill)
    paths = V.remap_tensors(CS.to_product(EQUI_SPEC), [up(img)], [dst], radius=30.0, interpolation=interp, boarder_mode=border,
                            boarder_value=BORDER_VALUE, chromatic=ca)
    got = dst.cpu().numpy()
    assert paths == ["ray"] and R.last_launch_kinds() == ["chroma"], (paths, R.last_launch_kinds())
    assert np.array_equal(got, want), (interp, border, int((got != want).sum()))
    if border == 5:  # (the skipped bytes kept the pattern, channel by channel)
        assert (got == fill).any() and (got != fill).any()


def test_area_is_linear(V, ca, oracle_mod):
    img = noise(61, 83, 1)
    want, _ = expect(oracle_mod, EQUI_SPEC, img, size_output=(90, 70), radius=30.0, interp=1)
    dst = torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    V.remap_tensors(CS.to_product(EQUI_SPEC), [up(img)], [dst], radius=30.0, interpolation=3, chromatic=ca)
    assert np.array_equal(dst.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. ragged and tiny outputs: the npx edge, a second tile column one pixel wide, the last partial row group
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (255, 9), (257, 5), (333, 37)])
@pytest.mark.parametrize("interp", [1, 2])
def test_ragged_and_tiny_outputs(V, R, ca, oracle_mod, size, interp):
    img = noise(61, 83, 2)
    want, _ = expect(oracle_mod, EQUI_SPEC, img, size_output=size, radius=30.0, interp=interp, border=1)
    # the destination is a view inside a larger poisoned buffer: nothing outside the image may be written
    big = torch.full((size[1] + 2, size[0] + 5, 3), 0xA5, dtype=torch.uint8, device="cuda")
    dst = big[1:-1, 2:-3]
    V.remap_tensors(CS.to_product(EQUI_SPEC), [up(img)], [dst], radius=30.0, interpolation=interp, boarder_mode=1, chromatic=ca)
    # (the wide flat outputs are normalised by their height: their longitudes run far past the table, and a fix-up pass follows)
    kinds = R.last_launch_kinds()
    assert len(kinds) == 1 and kinds[0] in ("chroma", "chroma+fixup"), kinds
    assert np.array_equal(dst.cpu().numpy(), want)
    host = big.cpu().numpy()
    host[1:-1, 2:-3] = 0xA5
    assert (host == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. side-by-side pair: the second eye's rows start at byte 135 -- the byte store path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_side_by_side_pair_shared_and_per_eye(V, R, CA, ca, oracle_mod):
    O = oracle_mod
    left, right = noise(61, 83, 3), noise(61, 83, 4)
    t = CS.to_product(EQUI_SPEC)
    want = np.concatenate([expect(O, EQUI_SPEC, im, size_output=(45, 70), radius=30.0, interp=1)[0] for im in (left, right)], axis=1)
    out = V.apply_lr_tensors(t, up(left), up(right), size_output=(45, 70), interpolation=1, radius=30.0, chromatic=ca)
    assert out.shape == (70, 90, 3) and out[:, 45:].data_ptr() - out.data_ptr() == 135
    assert families(R.last_launch_kinds()) == ["chroma"]  # one launch of two units
    assert np.array_equal(out.cpu().numpy(), want)
    # (left, right): two plans
    other = {"b": [0, 1.003], "g": None, "r": [0, 0.996, 0, 0.004]}
    ca_r = CA.ChromaticAberration(red=other["r"], blue=other["b"])
    want2 = np.concatenate([expect(O, EQUI_SPEC, left, size_output=(45, 70), radius=30.0, interp=1)[0],
                            expect(O, EQUI_SPEC, right, size_output=(45, 70), radius=30.0, interp=1, coefs=other)[0]], axis=1)
    assert not np.array_equal(want2, want)
    out2 = V.apply_lr_tensors(t, up(left), up(right), size_output=(45, 70), interpolation=1, radius=30.0, chromatic=(ca, ca_r))
    assert families(R.last_launch_kinds()) == ["chroma", "chroma"]
    assert np.array_equal(out2.cpu().numpy(), want2)
    # radius="max" and an explicit centre go into every channel chain the same way
    out3 = V.apply_lr_tensors(t, up(left), up(right), size_output=(45, 70), interpolation=1, radius="max", chromatic=ca)
    want3 = np.concatenate([expect(O, EQUI_SPEC, im, size_output=(45, 70), radius=30.5, interp=1)[0] for im in (left, right)], axis=1)
    assert np.array_equal(out3.cpu().numpy(), want3)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. fused on every ray mode: classic without / with rotation, radial stages in front of a rotation, lat_x, planar
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_poly", "c4_rot_poly", "rot_after_radial", "equirect_lat_x", "transformer_poly", "transformer_rotator"])
def test_fused_on_every_ray_mode(V, R, CA, ca, oracle_mod, name):
    O = oracle_mod
    spec, out, inp, radius = CS.SMALL_CASES[name]
    assert max(out) <= 192
    t = CS.to_product(spec)
    img = noise(inp[0], inp[1], 5)
    want, _ = expect(O, spec, img, size_output=out, radius=radius, interp=1)
    dst = torch.zeros((out[1], out[0], 3), dtype=torch.uint8, device="cuda")
    paths = V.remap_tensors(t, [up(img)], [dst], radius=radius, interpolation=1, chromatic=ca)
    assert paths == ["ray"] and R.last_launch_kinds()[0].startswith("chroma"), (paths, R.last_launch_kinds())
    for c, s in zip("bgr", channel_specs(spec)):
        xm, ym = V.get_map(t, radius=radius, size_input=inp, size_output=out, chromatic=ca, channel=c)
        gx, gy = oracle_map(O, s, radius, inp, out)
        assert_maps_match(xm, ym, gx, gy, f"{name} channel {c}")
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), (name, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the fix-up pass
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,coefs", [("poly_c0", COEFS), ("back_hemisphere", COEFS),
                                        ("c2_poly", {"b": BLUE, "g": None, "r": [0.02, 1.004, 0, -0.006]})])
def test_fixup_pass(V, R, CA, oracle_mod, name, coefs):
    """poly_c0 and back_hemisphere at 512 as the parity tests run them; and a constant term in the red polynomial alone, so that one
    channel alone leaves its table near the centre (the whole pixel then takes the interpreter)"""
    spec = CS.SMALL_CASES[name][0]
    size = 512 if coefs is COEFS else 128
    img = noise(size, size, 6)
    want, _ = expect(oracle_mod, spec, img, size_output=(size, size), radius=size / 2, interp=1, coefs=coefs)
    dst = torch.zeros((size, size, 3), dtype=torch.uint8, device="cuda")
    paths = V.remap_tensors(CS.to_product(spec), [up(img)], [dst], radius=size / 2, interpolation=1,
                            chromatic=CA.ChromaticAberration(red=coefs["r"], blue=coefs["b"]))
    assert paths == ["ray"] and R.last_launch_kinds() == ["chroma+fixup"], (paths, R.last_launch_kinds())
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), (name, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. chains that do not fuse: three interpreters
# ---------------------------------------------------------------------------------------------------------------------------------
def test_literal_path(V, R, ca, oracle_mod):
    """An EquirectangularDecoder chain with the correction appended does not fuse: path 'literal', bytes equal.  `two_rotations` -- which
    the issue lists here -- composes its consecutive rotations into one matrix and takes the ray path as a single chain today, so by the
    fuse rule it fuses: asserted as such, bytes equal."""
    for name, want_path in (("equirect_decoder", "literal"), ("two_rotations", "ray")):
        spec, out, inp, radius = CS.SMALL_CASES[name]
        img = noise(inp[0], inp[1], 7)
        want, _ = expect(oracle_mod, spec, img, size_output=out, radius=radius, interp=1)
        dst = torch.zeros((out[1], out[0], 3), dtype=torch.uint8, device="cuda")
        paths = V.remap_tensors(CS.to_product(spec), [up(img)], [dst], radius=radius, interpolation=1, chromatic=ca)
        assert paths == [want_path] and families(R.last_launch_kinds()) == ["chroma"], (name, paths, R.last_launch_kinds())
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), (name, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. per-unit rotations=: two units with different matrices in one launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_per_unit_rotations(V, R, ca, oracle_mod):
    rots = [np.asarray(CS.ry(0.21)), np.asarray(CS.ry(-0.13)) @ np.asarray(CS.ry(0.05)).T]
    base = [("equirect_enc", True), ("rot", CS.ry(0.0)), ("poly", [0, 1, -0.1]), CS.EQUI]
    imgs = [noise(96, 96, 8), noise(96, 96, 9)]
    dsts = [torch.zeros((100, 120, 3), dtype=torch.uint8, device="cuda") for _ in imgs]
    paths = V.remap_tensors(CS.to_product(base), [up(i) for i in imgs], dsts, radius=48.0, interpolation=1, rotations=rots, chromatic=ca)
    assert paths == ["ray"] and len(R.last_launch_kinds()) == 1 and R.last_launch_kinds()[0].startswith("chroma")
    for k in range(2):
        spec = [base[0], ("rot", rots[k].tolist())] + base[2:]
        want, _ = expect(oracle_mod, spec, imgs[k], size_output=(120, 100), radius=48.0, interp=1)
        got = dsts[k].cpu().numpy()
        assert np.array_equal(got, want), (k, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the inputs an LDS-staged kernel would have to hand back to the global-memory sampler: a tile whose taps span the whole source,
#    tiles that straddle the source edge, a source that is not dword-aligned.  One family serves them all here: 'chroma'.
# ---------------------------------------------------------------------------------------------------------------------------------
def test_large_source_into_a_tiny_output(V, R, ca, oracle_mod):
    img = noise(1024, 1024, 21)
    want, _ = expect(oracle_mod, EQUI_SPEC, img, size_output=(32, 32), radius=512.0, interp=1)
    dst = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    paths = V.remap_tensors(CS.to_product(EQUI_SPEC), [up(img)], [dst], radius=512.0, interpolation=1, chromatic=ca)
    assert paths == ["ray"] and families(R.last_launch_kinds()) == ["chroma"], (paths, R.last_launch_kinds())
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("border", [2, 0])  # REFLECT, CONSTANT
def test_radius_beyond_the_source_tiles_straddle_its_edge(V, R, ca, oracle_mod, border):
    img = noise(61, 83, 22)
    want, plain = expect(oracle_mod, EQUI_SPEC, img, size_output=(90, 70), radius=50.0, interp=1, border=border, bval=BORDER_VALUE)
    # (the condition on the inputs: footprints on both sides of the source's edge -- under CONSTANT some pixels are the border colour)
    if border == 0:
        assert (plain == np.array(BORDER_VALUE, np.uint8)).all(axis=2).mean() > 0.05
    dst = torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    paths = V.remap_tensors(CS.to_product(EQUI_SPEC), [up(img)], [dst], radius=50.0, interpolation=1, boarder_mode=border,
                            boarder_value=BORDER_VALUE, chromatic=ca)
    assert paths == ["ray"] and families(R.last_launch_kinds()) == ["chroma"], (paths, R.last_launch_kinds())
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), (border, int((got != want).sum()))


def test_source_view_at_an_odd_address(V, R, ca, oracle_mod):
    img = noise(61, 83, 23)
    want, _ = expect(oracle_mod, EQUI_SPEC, img, size_output=(90, 70), radius=30.0, interp=1)
    flat = torch.full((61 * 83 * 3 + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    src = flat[1:].view(61, 83, 3)
    src.copy_(up(img))
    assert src.data_ptr() % 2 == 1
    dst = torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    paths = V.remap_tensors(CS.to_product(EQUI_SPEC), [src], [dst], radius=30.0, interpolation=1, chromatic=ca)
    assert paths == ["ray"] and families(R.last_launch_kinds()) == ["chroma"], (paths, R.last_launch_kinds())
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. equal to the engine itself, independent of the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_each_channel_equals_the_engines_own_remap_of_that_chain(V, ca):
    spec = CS.SMALL_CASES["c4_rot_poly"][0]
    t = CS.to_product(spec)
    img = up(noise(128, 128, 10))
    fused = torch.zeros((150, 170, 3), dtype=torch.uint8, device="cuda")
    V.remap_tensors(t, [img], [fused], radius=64.0, interpolation=1, chromatic=ca)
    plain = torch.zeros_like(fused)
    V.remap_tensors(t, [img], [plain], radius=64.0, interpolation=1)
    assert not torch.equal(fused, plain)
    for c, tc in enumerate(ca.channel_transformers(t)):
        one = torch.zeros_like(fused)
        V.remap_tensors(tc, [img], [one], radius=64.0, interpolation=1)
        assert torch.equal(fused[..., c], one[..., c]), c


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. graph capture
# ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay_on_new_contents(V, R, ca, oracle_mod):
    O = oracle_mod
    spec = CS.SMALL_CASES["c2_poly"][0]
    t = CS.to_product(spec)
    first, second = (noise(128, 128, 11), noise(128, 128, 12)), (noise(128, 128, 13), noise(128, 128, 14))
    left, right = up(first[0]), up(first[1])
    out = torch.zeros((96, 192, 3), dtype=torch.uint8, device="cuda")
    kw = dict(out=out, size_output=(96, 96), interpolation=1, radius=64.0, chromatic=ca)
    V.apply_lr_tensors(t, left, right, **kw)  # (the plan exists: creating one is not capturable)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        V.apply_lr_tensors(t, left, right, **kw)
    assert R.last_launch_kinds() == ["chroma"]  # one launch of two units: a single chain of nodes
    for a, b in (second, first):
        left.copy_(up(a)), right.copy_(up(b))
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = np.concatenate([expect(O, spec, im, size_output=(96, 96), radius=64.0, interp=1)[0] for im in (a, b)], axis=1)
        assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# the file-level entries and what composes with the remap's result
# ---------------------------------------------------------------------------------------------------------------------------------
def test_apply_and_apply_lr_with_arrays(V, ca, oracle_mod, tmp_path):
    O = oracle_mod
    imgs = [noise(61, 83, 15), noise(61, 83, 16)]
    res = V.apply(CS.to_product(EQUI_SPEC), in_paths=imgs, size_output=(90, 70), interpolation=1, radius=30.0, chromatic=ca)
    for im, got in zip(imgs, res):
        assert np.array_equal(np.asarray(got), expect(O, EQUI_SPEC, im, size_output=(90, 70), radius=30.0, interp=1)[0])
    # center= travels into every channel chain: compared with the engine's own remap of each chain (the oracle's spec has no centre)
    t = CS.to_product(EQUI_SPEC)
    src = up(imgs[0])
    fused = torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    V.remap_tensors(t, [src], [fused], radius=30.0, interpolation=1, center=(43.25, 29.5), chromatic=ca)
    for c, tc in enumerate(ca.channel_transformers(t)):
        one = torch.zeros_like(fused)
        V.remap_tensors(tc, [src], [one], radius=30.0, interpolation=1, center=(43.25, 29.5))
        assert torch.equal(fused[..., c], one[..., c]), c
    # match_colors acts on the remap's result
    sbs = V.apply_lr_tensors(t, up(imgs[0]), up(imgs[1]), size_output=(45, 70), interpolation=1, radius=30.0, chromatic=ca)
    matched = V.apply_lr_tensors(t, up(imgs[0]), up(imgs[1]), size_output=(45, 70), interpolation=1, radius=30.0, chromatic=ca,
                                 match_colors="gain")
    from vr180_convert_amd import colormatch

    ref = sbs.clone()
    colormatch.match_eyes_tensors(ref[:, :45], ref[:, 45:], mode="gain", reference="left")
    assert torch.equal(matched, ref)


def test_c_abi_argument_errors(V, CA, ca):
    """argument errors of v1c_ca_plan_run are reported before anything is launched"""
    import ctypes as C

    from vr180_convert_amd import _abi, _native

    chains = CA.lower_channels(CS.to_product(EQUI_SPEC), ca, radius=30.0, size_input=(61, 83), size_output=(90, 70))
    plan = CA.CaPlan(chains, src_hw=(61, 83), dst_wh=(90, 70), interpolation=1, border_mode=0, border_value=0, device="cuda")
    assert plan.path == "ray" and plan.last_launch() == ""
    L = _native.lib()
    units = (_abi.Unit * 1)()
    assert L.v1c_ca_plan_run(plan._h, None, units, 1) == _abi.E_INVALID  # NULL src / dst
    src, dst = torch.zeros((61, 83, 3), dtype=torch.uint8, device="cuda"), torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    units[0].src, units[0].dst, units[0].src_pitch, units[0].dst_pitch = src.data_ptr(), dst.data_ptr(), 83 * 3 - 1, 270
    assert L.v1c_ca_plan_run(plan._h, None, units, 1) == _abi.E_INVALID  # pitch below a row
    units[0].src_pitch, units[0].has_rot = 83 * 3, 1
    assert L.v1c_ca_plan_run(plan._h, None, units, 1) == _abi.E_INVALID  # a rotation for chains without a rotate stage
    assert L.v1c_ca_plan_run(plan._h, None, units, 0) == _abi.E_INVALID
    assert L.v1c_ca_plan_get_map(plan._h, None, 3, dst.data_ptr(), dst.data_ptr(), 360, None) == _abi.E_INVALID
    assert plan.last_launch() == ""
    h = C.c_void_p()
    bad = (_abi.Chain * 3)(*chains)
    bad[2].n_ops = 0
    assert L.v1c_ca_plan_create(C.byref(h), 0, bad, 61, 83, 70, 90, 1, 0, None) == _abi.E_INVALID and not h
    # more than 16 units: several launches
    n = 19
    srcs = [up(noise(61, 83, 20 + k)) for k in range(n)]
    dsts = [torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
    plan.run(srcs, dsts)
    one = torch.zeros((70, 90, 3), dtype=torch.uint8, device="cuda")
    for k in (0, 15, 16, 18):
        plan.run([srcs[k]], [one])
        assert torch.equal(one, dsts[k]), k
