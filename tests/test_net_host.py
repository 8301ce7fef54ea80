"""CPU: a whole fused evaluation network in one library call (cimq_net_abi / cimq_net_sizes / cimq_net_forward) as
the host sees it -- the availability symbol, the layout of the three plan structs, the sizes a plan reports, every
refusal that needs no device (the plan is validated completely before the first launch, so a refused plan with
made-up addresses touches nothing), and FusedEval's slot assignment."""
import ctypes
import os
import subprocess

import pytest

from conftest import REPO
from test_inference_host import INF, case_desc

import cim_quantization_amd._lib as L
from cim_quantization_amd import build as cimq_build


@pytest.fixture(scope="module")
def lib():
    cimq_build.build(verbose=False)
    return L.load()


def test_net_abi(lib):
    assert lib.cimq_net_abi() == 1
    assert lib.cimq_abi_version() == 16 and lib.cimq_abi_minor() == 1  # (both unchanged)
    assert {"cimq_net_abi", "cimq_net_sizes", "cimq_net_forward"} <= set(L.EXPORTED_SYMBOLS)


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the three plan structs from gcc on include/cimq.h equal the ctypes mirrors"""
    mirrors = {"cimq_net_layer": L.NetLayer, "cimq_net_head": L.NetHead, "cimq_net_desc": L.NetDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cimq.h"', 'int main(void) {',
             '  printf("maxc x %d\\n", CIMQ_NET_HEAD_MAX_C);']
    for cname, cls in mirrors.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, fname, v = line.split()
        if cname == "maxc":
            assert int(v) == L.NET_HEAD_MAX_C
        elif fname == "size":
            assert int(v) == ctypes.sizeof(mirrors[cname]), cname
        else:
            assert int(v) == getattr(mirrors[cname], fname).offset, (cname, fname)
        seen += 1
    assert seen == 1 + sum(1 + len(c._fields_) for c in mirrors.values())


# made-up device addresses, 16-byte aligned: every refusal below is decided on the host before anything is
# dereferenced or launched
A = 0x7000_0000_0000
X, LOGITS, WS = A + 0x100_0000, A + 0x200_0000, A + 0x300_0000


class Plan:
    """l1 -> l2s2 -> l2 at B = 1: layer 0 writes slot 0 as fp32 and as layer 1's codes, layer 1 reads the codes and
    writes slot 1, layer 2 reads slot 1, adds slot 0 as an option-A view (16 of 32 channels from channel 8, stride
    2) and writes slot 2; the head pools slot 2 into 10 classes.  ``edit(plan)`` changes it before it is packed."""

    def __init__(self, names=("l1", "l2s2", "l2"), n_slots=3, head=True):
        self.descs = [case_desc(n, INF) for n in names]
        self.lsqs = [L.make_lsq_desc(-4, 3, 1e-3, 1e-3, 8) for _ in names]
        self.layers = (L.NetLayer * max(len(names), 1))()
        for i, lay in enumerate(self.layers[:len(names)]):
            base = A + 0x1000_0000 * (i + 1)
            (lay.weight, lay.alpha_act, lay.alpha_weight, lay.alpha_cim, lay.binary_mask, lay.signed_act, lay.scale,
             lay.shift, lay.ctx) = [base + 0x10_0000 * k for k in range(1, 10)]
            lay.beta_cim = None
            lay.epi_flags = L.CIMQ_EPI_RELU
            lay.in_slot, lay.in_codes, lay.out_slot, lay.out_mode, lay.consumer = i - 1, 0, i, 1, 0
            lay.res_slot, lay.res_c0, lay.res_stride, lay.reserved = -1, 0, 1, 0
        if names == ("l1", "l2s2", "l2"):
            self.layers[0].out_mode, self.layers[0].consumer = 3, 1
            self.layers[1].in_codes = 1
            self.layers[2].res_slot, self.layers[2].res_c0, self.layers[2].res_stride = 0, 8, 2
        self.head = L.NetHead()
        self.head.in_slot, self.head.classes = len(names) - 1, 10
        self.head.weight, self.head.bias, self.head.pooled = A + 0x400_0000, A + 0x500_0000, None
        self.has_head = head
        self.n_layers, self.n_slots = len(names), n_slots
        d0 = self.descs[0] if names else None
        self.shape = (d0.batch, d0.in_channels, d0.in_h, d0.in_w) if names else (2, 64, 8, 8)
        self.sf = [A + 0x6000_0000 + 0x100_0000 * k for k in range(8)]
        self.sc = [A + 0x7000_0000 + 0x100_0000 * k for k in range(8)]
        self.x, self.logits, self.ws = X, LOGITS, WS
        self.null_layers = self.null_slots = False

    def pack(self):
        for i in range(self.n_layers if self.n_layers > 0 else 0):
            if self.descs[i] is not None:
                self.layers[i].desc = ctypes.pointer(self.descs[i])
            if self.lsqs[i] is not None:
                self.layers[i].lsq = ctypes.pointer(self.lsqs[i])
        net = L.NetDesc()
        net.n_layers, net.n_slots = self.n_layers, self.n_slots
        net.layers = None if self.null_layers else ctypes.cast(self.layers, ctypes.POINTER(L.NetLayer))
        net.head = ctypes.pointer(self.head) if self.has_head else None
        net.B, net.C, net.H, net.W = self.shape
        return net

    def forward(self, lib):
        net = self.pack()
        n = max(self.n_slots, 1)
        sf, sc = (ctypes.c_void_p * n)(*self.sf[:n]), (ctypes.c_void_p * n)(*self.sc[:n])
        if self.null_slots:
            sf = sc = None
        return lib.cimq_net_forward(ctypes.byref(net), self.x, sf, sc, self.logits, self.ws, None)

    def sizes(self, lib):
        net = self.pack()
        n = max(self.n_slots, 1)
        fb, cb, ws = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), ctypes.c_size_t()
        rc = lib.cimq_net_sizes(ctypes.byref(net), fb, cb, ctypes.byref(ws))
        return rc, list(fb), list(cb), ws.value


def _refused(lib, edit, code, word=b"", **kw):
    p = Plan(**kw)
    edit(p)
    rc = p.forward(lib)
    msg = lib.cimq_last_error()
    assert rc == code, (rc, msg)
    assert msg and word in msg, msg
    return p


def _in_slot1(v):
    """layer 1 reads slot v as fp32 (and layer 0 writes no codes, which would name layer 1 their consumer)"""
    def edit(p):
        p.layers[0].out_mode, p.layers[1].in_codes, p.layers[1].in_slot = 1, 0, v
    return edit


def test_sizes_three_layer_plan(lib):
    p = Plan()
    rc, fb, cb, ws = p.sizes(lib)
    assert rc == 0, lib.cimq_last_error()
    # B * O * Ho * Wo * 4 per float plane, B * O * Ho * Wo per code plane, 0 where a plane is never stored
    assert fb == [1 * 16 * 32 * 32 * 4, 1 * 32 * 16 * 16 * 4, 1 * 32 * 16 * 16 * 4]
    assert cb == [1 * 16 * 32 * 32, 0, 0]
    assert ws == max(L.query_sizes(d).fwd_workspace_bytes for d in p.descs)
    # a slot used twice reports its largest plane: layer 2 writes into slot 0's place once slot 0 is dead
    q = Plan()
    q.layers[2].res_slot = -1
    q.layers[2].out_slot = 0
    q.head.in_slot = 0
    rc, fb, cb, ws = q.sizes(lib)
    assert rc == 0, lib.cimq_last_error()
    assert fb == [max(16 * 32 * 32, 32 * 16 * 16) * 4, 32 * 16 * 16 * 4, 0] and cb == [16 * 32 * 32, 0, 0]
    # the general route's workspace holds its [B, P, O] plane: the maximum over the layers is that layer's
    g = Plan(names=("c48", "c48"), n_slots=2)
    rc, fb, cb, ws = g.sizes(lib)
    assert rc == 0, lib.cimq_last_error()
    assert ws == L.query_sizes(g.descs[0]).fwd_workspace_bytes >= 4 * 48 * 16 * 16
    # either output array may be NULL
    net = p.pack()
    w = ctypes.c_size_t()
    assert lib.cimq_net_sizes(ctypes.byref(net), None, None, ctypes.byref(w)) == 0 and w.value == p.sizes(lib)[3]
    # a head-only plan needs no workspace
    h = Plan(names=(), n_slots=0)
    h.head.in_slot = -1
    rc, _, _, ws = h.sizes(lib)
    assert rc == 0 and ws == 0, lib.cimq_last_error()


def test_refuses_null_pointers(lib):
    assert lib.cimq_net_forward(None, X, None, None, LOGITS, WS, None) == L.CIMQ_EINVAL
    assert b"null plan" in lib.cimq_last_error()
    assert lib.cimq_net_sizes(None, None, None, None) == L.CIMQ_EINVAL
    _refused(lib, lambda p: setattr(p, "null_layers", True), L.CIMQ_EINVAL, b"null layers")
    _refused(lib, lambda p: setattr(p, "x", None), L.CIMQ_EINVAL, b"null x")
    _refused(lib, lambda p: setattr(p, "ws", None), L.CIMQ_EINVAL, b"null workspace")
    _refused(lib, lambda p: setattr(p, "logits", None), L.CIMQ_EINVAL, b"null logits")
    _refused(lib, lambda p: setattr(p, "null_slots", True), L.CIMQ_EINVAL, b"null slot arrays")
    _refused(lib, lambda p: p.descs.__setitem__(1, None), L.CIMQ_EINVAL, b"null descriptor")
    _refused(lib, lambda p: p.lsqs.__setitem__(2, None), L.CIMQ_EINVAL, b"null descriptor")
    _refused(lib, lambda p: p.sf.__setitem__(1, None), L.CIMQ_EINVAL, b"slot buffer")
    _refused(lib, lambda p: p.sc.__setitem__(0, None), L.CIMQ_EINVAL, b"slot buffer")
    _refused(lib, lambda p: setattr(p.head, "weight", None), L.CIMQ_EINVAL, b"null weight")
    # the per-layer call's own pointers, in any layer: found before the first launch
    for i in range(3):
        for field in ("weight", "alpha_act", "alpha_weight", "binary_mask", "signed_act", "ctx"):
            # (layer 1's alpha_act is also what layer 0 writes its codes with: that call refuses it first)
            word = b"out_alpha_act" if (i, field) == (1, "alpha_act") else b"null pointer"
            _refused(lib, lambda p: setattr(p.layers[i], field, None), L.CIMQ_EINVAL, word)
        _refused(lib, lambda p: setattr(p.layers[i], "alpha_cim", None), L.CIMQ_EINVAL, b"alpha_cim")
        _refused(lib, lambda p: setattr(p.layers[i], "scale", None), L.CIMQ_EINVAL, b"null epilogue")


def test_refuses_bad_counts(lib):
    _refused(lib, lambda p: setattr(p, "n_layers", -1), L.CIMQ_EINVAL, b"negative")
    _refused(lib, lambda p: setattr(p, "n_slots", -2), L.CIMQ_EINVAL, b"negative")
    _refused(lib, lambda p: None, L.CIMQ_EINVAL, b"without a head", names=(), n_slots=0, head=False)


def test_refuses_slot_index_out_of_range(lib):
    for v in (3, 7, -2):
        _refused(lib, _in_slot1(v), L.CIMQ_EINVAL, b"out of range")
        _refused(lib, lambda p: setattr(p.layers[1], "out_slot", v), L.CIMQ_EINVAL, b"out of range")
        _refused(lib, lambda p: setattr(p.layers[2], "res_slot", v), L.CIMQ_EINVAL, b"out of range")
        _refused(lib, lambda p: setattr(p.head, "in_slot", v), L.CIMQ_EINVAL, b"out of range")
    _refused(lib, lambda p: setattr(p.layers[0], "out_slot", -1), L.CIMQ_EINVAL, b"out of range")


def test_refuses_reading_what_nobody_wrote(lib):
    _refused(lib, _in_slot1(2), L.CIMQ_EINVAL, b"no earlier layer wrote")

    def float_only(p):  # layer 0 writes no codes, layer 1 still reads them
        p.layers[0].out_mode = 1
    _refused(lib, float_only, L.CIMQ_EINVAL, b"no earlier layer wrote")

    def codes_only(p):  # layer 0 writes no fp32, layer 2's residual still reads it
        p.layers[0].out_mode = 2
    _refused(lib, codes_only, L.CIMQ_EINVAL, b"no earlier layer wrote")

    def fp32_of_codes(p):  # ... and so does a layer that reads the slot as fp32
        p.layers[0].out_mode = 2
        p.layers[1].in_codes = 0
        p.layers[2].res_slot = -1
    _refused(lib, fp32_of_codes, L.CIMQ_EINVAL, b"no earlier layer wrote")
    _refused(lib, lambda p: setattr(p.layers[2], "res_slot", 2), L.CIMQ_EINVAL)  # (its own out_slot)

    def res_unwritten(p):
        p.n_slots = 4
        p.layers[2].res_slot = 3
    _refused(lib, res_unwritten, L.CIMQ_EINVAL, b"no earlier layer wrote")

    def head_unwritten(p):
        p.n_slots = 4
        p.head.in_slot = 3
    _refused(lib, head_unwritten, L.CIMQ_EINVAL, b"no earlier layer wrote")
    _refused(lib, lambda p: setattr(p.layers[0], "in_codes", 1), L.CIMQ_EINVAL, b"no code plane")

    def codes_for_another(p):  # slot 0's codes are layer 1's; layer 2 reads them
        p.layers[1].in_codes = 0
        p.layers[2].in_slot, p.layers[2].in_codes, p.layers[2].res_slot = 0, 1, -1
    _refused(lib, codes_for_another, L.CIMQ_EINVAL)


def test_refuses_shape_mismatch(lib):
    def consumer_shape(p):  # layer 1 now expects [1, 32, 16, 16], slot 0 holds [1, 16, 32, 32]
        p.descs[1] = case_desc("l2", INF)
    _refused(lib, consumer_shape, L.CIMQ_EINVAL, b"shape")
    _refused(lib, lambda p: setattr(p, "shape", (2, 16, 32, 32)), L.CIMQ_EINVAL, b"shape")
    _refused(lib, lambda p: setattr(p, "shape", (1, 16, 32, 31)), L.CIMQ_EINVAL, b"shape")


def test_refuses_out_slot_aliasing(lib):
    _refused(lib, lambda p: setattr(p.layers[1], "out_slot", 0), L.CIMQ_EINVAL, b"its own in_slot or res_slot")
    _refused(lib, lambda p: setattr(p.layers[2], "out_slot", 0), L.CIMQ_EINVAL, b"its own in_slot or res_slot")
    _refused(lib, lambda p: setattr(p.layers[2], "out_slot", 1), L.CIMQ_EINVAL, b"its own in_slot or res_slot")


def test_refuses_bad_consumer_and_modes(lib):
    for c in (0, 3, -1, 2):  # itself, past the end, before it, a later layer that reads another slot
        _refused(lib, lambda p: setattr(p.layers[0], "consumer", c), L.CIMQ_EINVAL, b"consumer")
    for mode in (0, 4, -1):
        _refused(lib, lambda p: setattr(p.layers[1], "out_mode", mode), L.CIMQ_EINVAL, b"out_mode")
    for v in (2, -1):
        _refused(lib, lambda p: setattr(p.layers[1], "in_codes", v), L.CIMQ_EINVAL, b"in_codes")


def test_refuses_bad_residual(lib):
    for s in (0, 3, -1, 4):
        _refused(lib, lambda p: setattr(p.layers[2], "res_stride", s), L.CIMQ_EINVAL, b"res_stride")
    # [32, 32] at stride 1 is not the output's [16, 16]
    _refused(lib, lambda p: setattr(p.layers[2], "res_stride", 1), L.CIMQ_EINVAL, b"residual source")
    for c0 in (-1, 17, 32):
        _refused(lib, lambda p: setattr(p.layers[2], "res_c0", c0), L.CIMQ_EINVAL, b"res_c0")
    for c0 in (0, 16):  # (the view at either edge of the 32 output channels is a valid plan)
        p = Plan()
        p.layers[2].res_c0 = c0
        assert p.sizes(lib)[0] == 0, lib.cimq_last_error()


def test_refuses_reserved(lib):
    for i in range(3):
        _refused(lib, lambda p: setattr(p.layers[i], "reserved", 1), L.CIMQ_EINVAL, b"reserved")
    _refused(lib, lambda p: p.head.reserved.__setitem__(0, 1), L.CIMQ_EINVAL, b"reserved")
    _refused(lib, lambda p: p.head.reserved.__setitem__(1, -1), L.CIMQ_EINVAL, b"reserved")
    _refused(lib, lambda p: setattr(p.head, "classes", 0), L.CIMQ_EINVAL, b"classes")


def test_refuses_what_the_layer_call_refuses(lib):
    def training_desc(p):
        p.descs[1] = case_desc("l2s2", 0)
    _refused(lib, training_desc, L.CIMQ_EINVAL, b"CIMQ_OPT_INFERENCE")
    _refused(lib, lambda p: setattr(p.layers[2], "epi_flags", 2), L.CIMQ_EINVAL, b"unknown flags")
    for off in (4, 8):
        _refused(lib, lambda p: p.sc.__setitem__(0, p.sc[0] + off), L.CIMQ_EINVAL, b"aligned")
        _refused(lib, lambda p: p.sf.__setitem__(0, p.sf[0] + off), L.CIMQ_EINVAL, b"aligned")
        _refused(lib, lambda p: setattr(p, "x", X + off), L.CIMQ_EINVAL, b"aligned")

    def overlapping(p):  # layer 2's out plane lies inside the tensor its residual view reads
        p.sf[2] = p.sf[0] + 256
    _refused(lib, overlapping, L.CIMQ_EINVAL, b"overlaps")

    def bad_lsq(p):
        p.lsqs[2] = L.make_lsq_desc(3, -4, 1e-3, 1e-3, 8)
    _refused(lib, bad_lsq, L.CIMQ_EINVAL, b"LSQ")


def test_unsupported_answers(lib):
    def qp255(p):  # the consumer's Qp leaves no byte for the NaN code
        p.descs[1] = case_desc("l2s2", INF, lsq_qp=255.0)
    _refused(lib, qp255, L.CIMQ_EUNSUPPORTED, b"lsq_qp")

    def stochastic(p):
        p.descs[1] = case_desc("l2s2", INF, adc_variant=L.CIMQ_ADC_STOCHASTIC)
    _refused(lib, stochastic, L.CIMQ_EUNSUPPORTED, b"stochastic")

    def dense_codes(p):
        p.layers[0].out_mode, p.layers[0].consumer = 3, 1
    _refused(lib, dense_codes, L.CIMQ_EUNSUPPORTED, b"dense", names=("dense", "dense"), n_slots=2)

    def dense_view(p):  # stride 2 over a 1 x 1 map: the same element, but a view all the same
        p.n_slots = 3
        p.layers[1].res_slot, p.layers[1].res_stride, p.layers[1].out_slot = 0, 2, 2
        p.head.in_slot = 2
    _refused(lib, dense_view, L.CIMQ_EUNSUPPORTED, b"dense", names=("dense", "dense"), n_slots=2)

    def wide_head(p):
        p.shape = (2, L.NET_HEAD_MAX_C + 1, 2, 2)
        p.head.in_slot = -1
    _refused(lib, wide_head, L.CIMQ_EUNSUPPORTED, b"CIMQ_NET_HEAD_MAX_C", names=(), n_slots=0)
    # cimq_net_sizes answers the same
    p = Plan()
    stochastic(p)
    assert p.sizes(lib)[0] == L.CIMQ_EUNSUPPORTED and b"stochastic" in lib.cimq_last_error()


def test_slot_assignment_resnet20():
    """three slots, each value in one slot from its write to its last read, and no step's output in a slot that
    holds a value still to be read (or read by that very step)"""
    from cim_quantization_amd.harness.fuse import assign_slots, resnet_steps
    for blocks in (3, 5):
        steps = resnet_steps(blocks)
        assert len(steps) == 6 * blocks + 2
        slot_of, n = assign_slots(steps)
        assert n == 3 and set(slot_of) == set(range(6 * blocks + 1)) and set(slot_of.values()) == {0, 1, 2}
        last = {}
        for t, (reads, _) in enumerate(steps):
            for v in reads:
                last[v] = t
        holder = {}
        for t, (reads, write) in enumerate(steps):
            for v in reads:
                assert holder[slot_of[v]] == v, (t, v)  # what a step reads is still where it was written
            if write is None:
                continue
            s = slot_of[write]
            assert s not in {slot_of[v] for v in reads}
            assert s not in holder or last[holder[s]] < t, (t, write)
            holder[s] = write
    # a chain with no shortcuts needs two
    chain = [((), 0)] + [((i,), i + 1) for i in range(6)] + [((6,), None)]
    assert assign_slots(chain)[1] == 2
