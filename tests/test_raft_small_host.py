"""RAFT-small without a GPU: the module tree and its state_dict, the two new C entry points, what CorrBlock accepts.

The counts are the reference's own: RAFT(small=True) there has 106 state_dict entries and 990 162 parameters
(tests/golden/make_raft_small_golden.py asserts both when it builds the fixtures)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("accflow_corr_lookup_r3_f32", "accflow_upflow8_f32")


def small():
    from accflow_amd.networks.raft.raft import RAFT, small_args
    return RAFT(small_args())


def test_raft_small_constructs_with_the_reference_state_dict():
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.raft.extractor import BottleneckBlock, SmallEncoder
    from accflow_amd.networks.raft.update import ConvGRU, SmallMotionEncoder, SmallUpdateBlock
    m = small()
    assert (m.hidden_dim, m.context_dim, m.args.corr_levels, m.args.corr_radius) == (96, 64, 4, 3)
    assert isinstance(m.fnet, SmallEncoder) and isinstance(m.cnet, SmallEncoder) and isinstance(m.update_block, SmallUpdateBlock)
    assert (m.fnet.norm_fn, m.cnet.norm_fn) == ("instance", "none")
    assert isinstance(m.fnet.layer2[0], BottleneckBlock) and m.fnet.layer2[0].downsample is not None
    assert isinstance(m.update_block.gru, ConvGRU) and isinstance(m.update_block.encoder, SmallMotionEncoder)
    assert not hasattr(m.update_block, "mask")
    sd = m.state_dict()
    assert len(sd) == 106
    assert sum(p.numel() for p in m.parameters()) == 990162
    shapes = {"fnet.conv1.weight": (32, 3, 7, 7), "fnet.layer2.0.conv2.weight": (16, 16, 3, 3),
              "fnet.layer2.0.downsample.0.weight": (64, 32, 1, 1), "fnet.conv2.weight": (128, 96, 1, 1),
              "cnet.conv2.weight": (160, 96, 1, 1), "update_block.encoder.convc1.weight": (96, 196, 1, 1),
              "update_block.encoder.convf1.weight": (64, 2, 7, 7), "update_block.encoder.convf2.weight": (32, 64, 3, 3),
              "update_block.encoder.conv.weight": (80, 128, 3, 3), "update_block.gru.convz.weight": (96, 242, 3, 3),
              "update_block.gru.convq.bias": (96,), "update_block.flow_head.conv1.weight": (128, 96, 3, 3),
              "update_block.flow_head.conv2.weight": (2, 128, 3, 3)}
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    # a strict load of a dict with exactly these keys and shapes (what a raft-small checkpoint holds) round-trips
    new = make_state_dict(m)
    m2 = small()
    m2.load_state_dict(new, strict=True)
    assert all(torch.equal(m2.state_dict()[k], new[k]) for k in new)
    m.load_state_dict(m2.state_dict(), strict=True)


def test_full_raft_and_the_builder_are_unchanged():
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.raft.raft import RAFT, default_args, small_args
    assert small_args().small is True and default_args().small is False
    full = build_flow_estimator("raft")
    assert isinstance(full, RAFT) and not full.small and full.args.corr_radius == 4 and full.hidden_dim == 128
    assert not full._packs_usable({}, []) and not small()._packs_usable({"fmap_base": (torch.zeros(2, 128, 16, 24), {0: 0, 1: 1})},
                                                                       [(0, 1)])


def test_new_entry_points_are_declared_exported_and_reject_null():
    from accflow_amd import _lib
    header = open(os.path.join(ROOT, "include", "accflow_hip.h")).read()
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert callable(getattr(lib, name))          # (the .so exports it: ctypes resolves the symbol here)
    assert _lib.SIGNATURES["accflow_corr_lookup_r3_f32"] == _lib.SIGNATURES["accflow_corr_lookup_f32"]
    assert lib.accflow_abi_version() == 20
    assert lib.accflow_corr_lookup_r3_f32(z, z, z, z, z, z, 0, 1, 16, 32, z) == 1
    assert lib.accflow_upflow8_f32(z, 0, z, 0, 1, 16, 32, z) == 1
    nz = ctypes.c_void_p(256)                        # (never dereferenced: the size checks come first)
    assert lib.accflow_corr_lookup_r3_f32(nz, nz, nz, nz, nz, nz, 0, 0, 16, 32, z) == 1
    assert lib.accflow_corr_lookup_r3_f32(nz, nz, nz, nz, nz, nz, 0, 1, 7, 32, z) == 1
    assert lib.accflow_upflow8_f32(nz, 0, nz, 0, 0, 16, 32, z) == 1
    assert lib.accflow_upflow8_f32(nz, 0, nz, 0, 1, 0, 32, z) == 1
    assert lib.accflow_upflow8_f32(nz, 0, nz, 0, 1, 16, -1, z) == 1
    assert lib.accflow_upflow8_f32(nz, 0, ctypes.c_void_p(260), 0, 1, 16, 32, z) == 1     # out not 16-byte aligned


def test_corr_block_radii():
    from accflow_amd.networks.raft.corr import AlternateCorrBlock, CorrBlock
    f = torch.zeros(1, 128, 16, 24)
    with pytest.raises(RuntimeError, match="MI355X"):        # radius 3 is accepted: the next refusal is the CPU tensor
        CorrBlock(f, f, radius=3)
    with pytest.raises(NotImplementedError):
        CorrBlock(f, f, radius=2)
    with pytest.raises(NotImplementedError):
        AlternateCorrBlock(f, f, radius=3)
    m = small()
    m.args.alternate_corr = True
    with pytest.raises(NotImplementedError):
        m._alternate()


def test_other_norms_keep_raising():
    from accflow_amd.networks.raft.extractor import SmallEncoder
    for kind in ("group", "batch"):
        enc = SmallEncoder(output_dim=128, norm_fn=kind).eval()
        with pytest.raises(NotImplementedError):
            enc(torch.zeros(1, 3, 64, 64))
