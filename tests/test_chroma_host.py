"""Host side of the chromatic-aberration remap (vr180_convert_amd/chromatic.py, csrc/chroma_plan.hpp, csrc/chroma_core.hpp): the channel
chains, the plan keys, ``--chromatic``, what is refused before the engine is touched, which chains fuse, and the host build of
``ray_eval3`` against ``ray_eval`` bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import chainspecs as CS
import vr180_convert_amd as V
import vr180_convert_amd.transformer as T
from vr180_convert_amd import _abi, _native, chromatic as CA, cli

RED = [0, 1.004, 0, -0.006]
BLUE = [0, 0.997, 0, 0.005]


def base():
    return T.EquirectangularEncoder() * T.FisheyeDecoder("equidistant")


# ---------------------------------------------------------------------------------------------------------------------------------
# the object and its chains
# ---------------------------------------------------------------------------------------------------------------------------------
def test_channel_chains_carry_the_stage_last_and_identity_appends_nothing():
    ca = CA.ChromaticAberration(red=RED, blue=BLUE)
    t = base()
    tb, tg, tr = ca.channel_transformers(t)
    assert tg is t
    for tc, coefs in ((tb, BLUE), (tr, RED)):
        assert tc.transformers[:-1] == t.transformers
        assert isinstance(tc.transformers[-1], T.PolynomialScaler) and list(tc.transformers[-1].coefs_reverse) == coefs
    chains = CA.lower_channels(t, ca, radius=30.0, size_input=(61, 83), size_output=(90, 70))
    nb, ng, nr = (c.n_ops for c in chains)
    assert nb == nr == ng + 1
    for c, coefs in ((chains[0], BLUE), (chains[2], RED)):
        last, dn = c.ops[c.n_ops - 2], c.ops[c.n_ops - 1]
        assert dn.opcode == _abi.OP_DENORMALIZE  # the stage sits directly in front of the Denormalize get_map appends
        assert last.opcode == _abi.OP_RADIAL and last.iparam == _abi.RAD_POLYNOMIAL and list(last.p[: last.nparam]) == coefs
    # the plain chain is what the entry point without chromatic= lowers
    from vr180_convert_amd.chain import lower_for_get_map

    assert bytes(chains[1]) == bytes(lower_for_get_map(t, radius=30.0, size_input=(61, 83), size_output=(90, 70)))
    # None and the identity append nothing
    for ident in (CA.ChromaticAberration(), CA.ChromaticAberration(red=[0, 1], blue=None, green=[0.0, 1.0])):
        assert all(x is t for x in ident.channel_transformers(t))
        assert ident.key() == (None, None, None)
    # a centre goes into every channel chain the same way
    cc = CA.lower_channels(t, ca, radius=30.0, size_input=(61, 83), size_output=(90, 70), center=(40.25, 31.5))
    for c in cc:
        assert list(c.ops[c.n_ops - 1].p[:4]) == [30.0, 30.0, 40.25, 31.5]


def test_bad_coefficients_are_refused():
    for bad in ([], "abc", [0, float("nan")], [0.0] * 17):
        with pytest.raises(ValueError):
            CA.ChromaticAberration(red=bad)
    with pytest.raises(TypeError):
        CA.as_per_unit("r:0,1", 2)
    with pytest.raises(TypeError):
        CA.as_per_unit((CA.ChromaticAberration(),), 2)


def test_plan_keys():
    t = base()
    kw = dict(src_hw=(61, 83), dst_wh=(90, 70), interpolation=1, border_mode=0, border_value=0, device_index=0)

    def key(ca):
        return CA.plan_key(CA.lower_channels(t, ca, radius=30.0, size_input=(61, 83), size_output=(90, 70)), **kw)

    a, b = CA.ChromaticAberration(red=RED, blue=BLUE), CA.ChromaticAberration(red=list(RED), blue=tuple(BLUE))
    assert a == b and a.key() == b.key() and hash(a.key()) == hash(b.key()) and key(a) == key(b)
    c = CA.ChromaticAberration(red=[0, 1.004, 0, np.nextafter(-0.006, 0)], blue=BLUE)
    assert c.key() != a.key() and key(c) != key(a)
    assert key(CA.ChromaticAberration(red=BLUE, blue=RED)) != key(a)  # the channels are not interchangeable
    assert key(a) != CA.plan_key(CA.lower_channels(t, a, radius=30.0, size_input=(61, 83), size_output=(90, 70)), **{**kw, "interpolation": 2})


# ---------------------------------------------------------------------------------------------------------------------------------
# --chromatic
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_option_parsing():
    import typer

    ca = cli.parse_chromatic("r:0,1.0012,0,-0.0009;b:0,0.9991,0,0.0006")
    assert ca == CA.ChromaticAberration(red=[0, 1.0012, 0, -0.0009], blue=[0, 0.9991, 0, 0.0006])
    assert cli.parse_chromatic("") is None
    assert cli.parse_chromatic(" G : 0, 1.001 ; ") == CA.ChromaticAberration(green=[0, 1.001])
    pair = cli.parse_chromatic("r:0,1.001|b:0,0.999")
    assert pair == (CA.ChromaticAberration(red=[0, 1.001]), CA.ChromaticAberration(blue=[0, 0.999]))
    assert cli.parse_chromatic("r:0,1.001|b:0,0.999", swap=True) == (pair[1], pair[0])  # a per-eye pair swaps with the eyes
    assert cli.parse_chromatic("r:0,1.001", swap=True) == CA.ChromaticAberration(red=[0, 1.001])
    for bad in ("x:0,1", "r", "r:", "r:0,one", "r:0,1;r:0,1", ";", "r:0,1|b:0,1|g:0,1", "r:0,nan"):
        with pytest.raises(typer.BadParameter):
            cli.parse_chromatic(bad)
    with pytest.raises(typer.BadParameter):
        cli.parse_chromatic("r:0,1.001|b:0,0.999", pair=False)  # `s` remaps with one map


def test_cli_commands_have_the_option():
    from typer.testing import CliRunner

    for cmd in ("lr", "s"):
        r = CliRunner().invoke(cli.app, [cmd, "--help"], env={"COLUMNS": "200", "TERM": "dumb"})
        assert r.exit_code == 0 and "--chromatic" in r.output


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals, before the engine is touched
# ---------------------------------------------------------------------------------------------------------------------------------
class _Custom(T.TransformerBase):
    """a user stage: only a NumPy transform, no op form"""

    def transform(self, x, y, **kw):
        return x, y

    def inverse_transform(self, x, y, **kw):
        return x, y


@pytest.fixture
def no_engine(monkeypatch):
    def boom():
        raise AssertionError("the engine was touched before the refusal")

    monkeypatch.setattr(_native, "lib", boom)


def test_refusals_come_before_the_engine(no_engine):
    ca = CA.ChromaticAberration(red=RED, blue=BLUE)
    t = base()
    kw = dict(radius=30.0, interpolation=1)

    def im(cn=3, dtype=torch.uint8, hw=(61, 83)):
        return torch.zeros((*hw, cn), dtype=dtype)

    def out(cn=3, dtype=torch.uint8):
        return torch.zeros((70, 90, cn), dtype=dtype)

    for cn in (1, 4):
        with pytest.raises(ValueError, match="3-channel"):
            V.remap_tensors(t, [im(cn)], [out(cn)], chromatic=ca, **kw)
    for dt in (torch.uint16, torch.float32):
        with pytest.raises(TypeError, match="uint8"):
            V.remap_tensors(t, [im(3, dt)], [out(3, dt)], chromatic=ca, **kw)
    with pytest.raises(NotImplementedError, match="lowered"):
        V.remap_tensors(t * _Custom(), [im()], [out()], chromatic=ca, **kw)
    with pytest.raises(TypeError):
        V.remap_tensors(t, [im()], [out()], chromatic="r:0,1.001", **kw)
    # the pair entries
    with pytest.raises(NotImplementedError, match="auto"):
        V.apply_lr_tensors(t, im(), im(), size_output=(90, 70), radius="auto", auto_radius_on_device=True, chromatic=ca)
    with pytest.raises(ValueError, match="3-channel"):
        V.apply_lr_tensors(t, im(1), im(1), size_output=(90, 70), radius=30.0, chromatic=ca)
    with pytest.raises(TypeError, match="uint8"):
        V.apply_lr_tensors(t, im(3, torch.float32), im(3, torch.float32), size_output=(90, 70), radius=30.0, chromatic=(ca, ca))
    with pytest.raises(NotImplementedError, match="lowered"):
        V.apply_lr_tensors(t * _Custom(), im(), im(), out=torch.zeros((70, 180, 3), dtype=torch.uint8), size_output=(90, 70), radius=30.0,
                           chromatic=ca)
    # the file-level entries, on arrays
    gray, wide = np.zeros((61, 83), np.uint8), np.zeros((61, 83, 3), np.uint16)
    with pytest.raises(ValueError, match="3-channel"):
        V.apply(t, in_paths=[gray], size_output=(90, 70), radius=30.0, chromatic=ca)
    with pytest.raises(TypeError, match="uint8"):
        V.apply(t, in_paths=[wide], size_output=(90, 70), radius=30.0, chromatic=ca)
    bgr = np.zeros((61, 83, 3), np.uint8)
    with pytest.raises(TypeError, match="one ChromaticAberration"):  # (apply shares one map: no per-image list)
        V.apply(t, in_paths=[bgr, bgr], size_output=(90, 70), radius=30.0, chromatic=(ca, ca))
    with pytest.raises(ValueError, match="3-channel"):
        V.apply_lr(t, left_path=gray, right_path=gray, out_path=None, size_output=(90, 70), radius=30.0, chromatic=ca)
    with pytest.raises(TypeError, match="uint8"):
        V.apply_lr(t, left_path=wide, right_path=wide, out_path=None, size_output=(90, 70), radius=30.0, chromatic=ca)
    with pytest.raises(ValueError, match="go together"):
        V.get_map(t, radius=30.0, size_input=(61, 83), size_output=(90, 70), chromatic=ca)
    with pytest.raises(ValueError, match="channel"):
        V.get_map(t, radius=30.0, size_input=(61, 83), size_output=(90, 70), chromatic=ca, channel="x")
    with pytest.raises(NotImplementedError, match="lowered"):
        V.get_map(t * _Custom(), radius=30.0, size_input=(61, 83), size_output=(90, 70), chromatic=ca, channel="r")


def test_grouping_is_host_logic(no_engine):
    """one shared correction: one group of two units; (left, right) corrections: two groups; per-unit rotations travel with the units"""
    ca, cb = CA.ChromaticAberration(red=RED, blue=BLUE), CA.ChromaticAberration(red=BLUE)
    t = base()
    srcs = [torch.zeros((61, 83, 3), dtype=torch.uint8) for _ in range(2)]
    dsts = [torch.zeros((70, 90, 3), dtype=torch.uint8) for _ in range(2)]
    g = CA.group_units(t, srcs, dsts, ca, radius=30.0)
    assert len(g) == 1 and g[0].index == [0, 1] and g[0].rots is None and len(g[0].chains) == 3
    g = CA.group_units(t, srcs, dsts, (ca, cb), radius=30.0)
    assert [x.index for x in g] == [[0], [1]]
    tr = T.EquirectangularEncoder() * T.Euclidean3DRotator(np.asarray(CS.ry(0.1))) * T.FisheyeDecoder("equidistant")
    rots = [np.asarray(CS.ry(0.1)), np.asarray(CS.ry(-0.2))]
    g = CA.group_units(tr, srcs, dsts, ca, radius=30.0, rotations=rots)
    assert len(g) == 1 and len(g[0].rots) == 2 and np.allclose(np.asarray(g[0].rots[1]).reshape(3, 3), rots[1])
    for ch in g[0].chains:  # the plan's chains carry the blanked rotation
        rot_ops = [ch.ops[i] for i in range(ch.n_ops) if ch.ops[i].opcode == _abi.OP_ROTATE]
        assert len(rot_ops) == 1 and list(rot_ops[0].p[:9]) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    with pytest.raises(ValueError, match="Euclidean3DRotator"):
        CA.group_units(t, srcs, dsts, ca, radius=30.0, rotations=rots)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fuse rule and ray_eval3, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ca_emul(product_lib):
    from host_chroma.build import build

    return C.CDLL(str(build()))


def channel_chains(oracle_mod, name):
    spec, out, inp, radius = CS.SMALL_CASES[name]
    specs = [spec + [("poly", BLUE)], spec, spec + [("poly", RED)]]
    arr = (oracle_mod.Chain * 3)(*[oracle_mod.chain_from_spec(s, radius=radius, size_input=inp, size_output=out) for s in specs])
    return arr, out


def takes_ray_today(emul_lib, oracle_mod, name):
    spec, out, inp, radius = CS.SMALL_CASES[name]
    ch = oracle_mod.chain_from_spec(spec, radius=radius, size_input=inp, size_output=out)
    info = (C.c_longlong * 12)()
    assert emul_lib.emul_plan_info(C.byref(ch), out[0], out[1], info) == 0
    return bool(info[0] and info[1])  # analysed and usable


# The EquirectangularDecoder chains are the literal ones of SMALL_CASES.  (`two_rotations` is NOT: analyze_chain composes consecutive
# rotate stages into one matrix, its single-chain plan takes the ray path today -- takes_ray_today() below asks the plan logic --, and by the
# fuse rule it fuses like every other ray chain; only a per-unit rotation override sends it to the interpreter.)
LITERAL_TODAY = ["equirect_decoder", "equirect_decoder_lat_x"]


@pytest.mark.parametrize("name", list(CS.SMALL_CASES))
def test_fuse_rule_and_ray_eval3_bit_for_bit(ca_emul, emul_lib, oracle_mod, name):
    """Every chain of SMALL_CASES that takes the ray path today fuses with the two polynomials appended, and the host ray_eval3 gives,
    for every pixel at the case's size, what ray_eval gives with that channel's own plan: the same verdict (a pixel is valid only when
    all three channels are) and the same bits; the fused plan's tables are the single-chain plans' tables.  Chains that are literal today
    do not fuse."""
    arr, out = channel_chains(oracle_mod, name)
    info = (C.c_longlong * 5)()
    assert ca_emul.ca_emul_fuse(arr, out[0], out[1], info) == 0
    ray_today = takes_ray_today(emul_lib, oracle_mod, name)
    assert ray_today == (name not in LITERAL_TODAY), name
    if not ray_today:
        assert info[0] == 0, name
        return
    assert info[0] == 1 and list(info[1:4]) == [0, 1, 2] and info[4] == 1, (name, list(info))
    st = (C.c_longlong * 6)()
    assert ca_emul.ca_emul_compare(arr, out[0], out[1], st) == 0
    pixels, valid, verdict_diff, bit_diff, table_diff, _partial = list(st)
    assert pixels == out[0] * out[1]
    assert table_diff == 0 and verdict_diff == 0 and bit_diff == 0, (name, list(st))
    if name in ("c2_poly", "c4_rot_poly", "apply_equirectangular", "equirect_lat_x", "rot_after_radial", "transformer_poly"):
        assert valid == pixels, (name, list(st))  # (no fix-up pixels there)
    if name == "poly_c0":
        assert 0 < valid < pixels, (name, list(st))


def test_equal_composites_share_a_table(ca_emul, oracle_mod):
    spec, out, inp, radius = CS.SMALL_CASES["c2_poly"]
    mk = lambda s: oracle_mod.chain_from_spec(s, radius=radius, size_input=inp, size_output=out)  # noqa: E731
    info = (C.c_longlong * 5)()
    arr = (oracle_mod.Chain * 3)(mk(spec), mk(spec), mk(spec + [("poly", RED)]))
    assert ca_emul.ca_emul_fuse(arr, out[0], out[1], info) == 0 and list(info[:4]) == [1, 1, 1, 2]
    arr = (oracle_mod.Chain * 3)(mk(spec + [("poly", RED)]), mk(spec), mk(spec + [("poly", RED)]))
    assert ca_emul.ca_emul_fuse(arr, out[0], out[1], info) == 0 and list(info[:4]) == [1, 0, 1, 0]
    # chains that differ in more than the radial composite do not fuse: another radius, another rotation
    other = oracle_mod.chain_from_spec(spec, radius=radius + 1, size_input=inp, size_output=out)
    arr = (oracle_mod.Chain * 3)(other, mk(spec), mk(spec))
    assert ca_emul.ca_emul_fuse(arr, out[0], out[1], info) == 0 and info[0] == 0
    s4 = CS.SMALL_CASES["c4_rot_poly"][0]
    arr = (oracle_mod.Chain * 3)(mk(s4), mk([s4[0], ("rot", CS.ry(0.5))] + s4[2:]), mk(s4))
    assert ca_emul.ca_emul_fuse(arr, out[0], out[1], info) == 0 and info[0] == 0


def test_only_red_constant_term_invalidates_red_alone(ca_emul, oracle_mod):
    """a constant term in the red polynomial alone: near the centre red leaves its table where blue and green stay inside"""
    spec, out, inp, radius = CS.SMALL_CASES["c2_poly"]
    mk = lambda s: oracle_mod.chain_from_spec(s, radius=radius, size_input=inp, size_output=out)  # noqa: E731
    arr = (oracle_mod.Chain * 3)(mk(spec + [("poly", BLUE)]), mk(spec), mk(spec + [("poly", [0.02, 1.004, 0, -0.006])]))
    st = (C.c_longlong * 6)()
    assert ca_emul.ca_emul_compare(arr, out[0], out[1], st) == 0
    pixels, valid, verdict_diff, bit_diff, table_diff, partial = list(st)
    assert table_diff == 0 and verdict_diff == 0 and bit_diff == 0
    assert 0 < valid < pixels and partial > 0, list(st)
