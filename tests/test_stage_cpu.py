"""CPU: what the symbol-rate stages share (vit_vs_raw_iq_amd.stage) on a dummy subclass -- the frame check, the coercion of
per-frame side arguments, the result packing, the per-device table cache -- the class relationships of the three real stages, and
that every module which uses them imports on its own.  No GPU and no built library."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from vit_vs_raw_iq_amd import Carrier, Equaliser, IqError, LikelihoodClassifier
from vit_vs_raw_iq_amd.frontend import FrontEnd
from vit_vs_raw_iq_amd.stage import DeviceTables, Stage, integers, pack, reals, stage_for

B, LENGTH = 2, 3


class Dummy(Stage):
    LAYOUTS, reference = ("rows", "planar"), "dummy_reference"

    def __init__(self, layout):
        super().__init__(LENGTH, layout)
        self.table, self.other = np.arange(4, dtype=np.float32), np.arange(5, dtype=np.float32)


def test_the_frame_check_refuses_a_wrong_shape_in_both_layouts_and_a_cpu_tensor():
    with pytest.raises(ValueError, match=r"layout must be one of \('rows', 'planar'\), got 'frames'"):
        Dummy("frames")
    for layout, good, shape in (("rows", (B, LENGTH, 2), r"\('B', 3, 2\)"), ("planar", (B, 2, LENGTH), r"\('B', 2, 3\)")):
        dummy = Dummy(layout)
        assert dummy.frame_shape(B) == good and dummy.planar == (layout == "planar") and dummy.layout == layout
        for bad in (torch.zeros(B, good[2], good[1]), torch.zeros(B, 2, 2), torch.zeros(good[1:]), torch.zeros(good + (1,)),
                    np.zeros(good), [[0.0] * 2] * LENGTH):
            with pytest.raises(ValueError, match=rf"x must be a {shape} tensor \(layout '{layout}'\), got "):
                dummy._check(bad)
        with pytest.raises(ValueError, match=r"dout must be a .* tensor \(layout"):
            dummy._check_shape(torch.zeros(1), "dout")
        dummy._check_shape(torch.zeros(good))
        dummy._check_shape(torch.zeros((0,) + good[1:]))
        with pytest.raises(IqError, match=r"Dummy runs on the MI355X only: x is a CPU tensor and there is no CPU fallback "
                                          r"\(dummy_reference is the host definition used by the tests\)"):
            dummy._check(torch.zeros(good))


def test_integers_take_a_list_an_array_or_a_tensor_and_refuse_the_rest():
    for good in ([[1, 2], [3, 4]], np.array([[1, 2], [3, 4]], np.uint8), torch.tensor([[1, 2], [3, 4]], dtype=torch.int64)):
        t = integers(good, "fth", (B, 2))
        assert t.dtype == torch.int32 and t.device.type == "cpu" and t.tolist() == [[1, 2], [3, 4]]
    moved = integers(torch.tensor([[1, 2], [3, 4]]).t(), "fth", (B, 2), torch.device("cpu"))
    assert moved.is_contiguous() and moved.tolist() == [[1, 3], [2, 4]]
    assert integers([5, 6], "u", (B,), wrap=lambda a: (a % 4).astype(np.int32)).tolist() == [1, 2]
    for bad in (np.zeros((B, 2)), np.zeros((B, 2), bool), np.zeros((B, 2), complex), [["a", "b"]] * B, "ab", None, 1.5):
        with pytest.raises(TypeError, match="fth must be a tensor or an array of integers, got "):
            integers(bad, "fth", (B, 2))
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bool):
        with pytest.raises(TypeError, match=f"fth must hold integers, got dtype {dtype}"):
            integers(torch.zeros(B, 2, dtype=dtype), "fth", (B, 2))
    for bad in (np.zeros((B, 3), int), torch.zeros(B, dtype=torch.int32), 7, np.zeros((1, B, 2), int)):
        with pytest.raises(ValueError, match=r"fth must have shape \(2, 2\) = \(F, TH\) per frame, got \("):
            integers(bad, "fth", (B, 2), note=" = (F, TH) per frame")
    with pytest.raises(ValueError, match=r"u must have shape \(2,\), got \(3,\)"):
        integers([1, 2, 3], "u", (B,))

    def refuses(arr):
        raise ValueError("out of range")
    with pytest.raises(ValueError, match="out of range"):                   # the array's own check comes before its shape's
        integers([1, 2, 3], "u", (B,), wrap=refuses)


def test_reals_broadcast_a_number_take_a_list_an_array_or_a_tensor_and_refuse_the_rest():
    for good, want in ((0.5, [0.5, 0.5]), (3, [3.0, 3.0]), (np.float64(0.25), [0.25, 0.25]), ([1, 2.5], [1.0, 2.5]),
                       (np.array([1, 2], np.int16), [1.0, 2.0]), (torch.tensor(0.5), [0.5, 0.5]),
                       (torch.tensor([1, 2]), [1.0, 2.0]), (torch.tensor([1.0, 2.0], dtype=torch.float64), [1.0, 2.0])):
        for device in (None, torch.device("cpu")):
            t = reals(good, "sigma2", (B,), device)
            assert t.dtype == torch.float32 and t.shape == (B,) and t.tolist() == want
            assert device is None or t.is_contiguous()
    for bad in (np.zeros(B, bool), np.zeros(B, complex), 1j, True, ["a", "b"], "ab", None):
        with pytest.raises(TypeError, match="sigma2 must be a number, an array or a tensor of real numbers, got "):
            reals(bad, "sigma2", (B,))
    for dtype in (torch.bool, torch.complex64):
        with pytest.raises(TypeError, match=f"sigma2 must hold real numbers, got dtype {dtype}"):
            reals(torch.zeros(B, dtype=dtype), "sigma2", (B,))
    for bad in (np.zeros(3), torch.zeros(B, 1), [[1.0, 2.0]]):
        with pytest.raises(ValueError, match=r"sigma2 must be a number or have shape \(2,\), one value per frame, got \("):
            reals(bad, "sigma2", (B,), note=", one value per frame")


def test_reals_as_pairs_take_complex_values_and_refuse_integer_tensors_and_a_bare_number():
    shape, note = (B, LENGTH, 2), " = (re, im) per frame and tap"
    z = np.arange(B * LENGTH).reshape(B, LENGTH) * (1 + 2j)
    want = np.stack([z.real, z.imag], axis=-1).astype(np.float32)
    for good in (z, z.tolist(), want, want.astype(np.float64), want.astype(np.int64), torch.from_numpy(z),
                 torch.from_numpy(want), torch.from_numpy(want).double()):
        t = reals(good, "w", shape, torch.device("cpu"), note, pairs=True)
        assert t.dtype == torch.float32 and t.is_contiguous() and np.array_equal(t.numpy(), want)
    for bad in (np.zeros(shape, bool), [[["a"] * 2] * LENGTH] * B, None):
        with pytest.raises(TypeError, match="w must be a tensor or an array of numbers, got "):
            reals(bad, "w", shape, pairs=True)
    for dtype in (torch.int32, torch.int64, torch.bool):
        with pytest.raises(TypeError, match=f"w must hold real or complex numbers, got dtype {dtype}"):
            reals(torch.zeros(shape, dtype=dtype), "w", shape, pairs=True)
    for bad in (np.zeros((B, LENGTH)), torch.zeros(B, LENGTH + 1, 2), np.zeros((B, LENGTH, 2), complex), torch.zeros(1, *shape)):
        with pytest.raises(ValueError, match=r"w must have shape \(2, 3, 2\) = \(re, im\) per frame and tap, got \("):
            reals(bad, "w", shape, None, note, pairs=True)
    with pytest.raises(ValueError, match=r"w must have shape \(2, 3, 2\), got \(1,\)"):       # no broadcast of one number
        reals(1.0, "w", shape, pairs=True)


def test_pack_gives_a_bare_tensor_without_extras_and_a_tuple_in_order_with_them():
    a, b, c = torch.zeros(1), torch.ones(1), torch.full((1,), 2.0)
    assert pack(a) is a and pack(a, None) is a and pack(a, None, None) is a
    for args, want in (((a, b), (a, b)), ((a, None, c), (a, c)), ((a, b, None), (a, b)), ((a, c, b), (a, c, b))):
        got = pack(*args)
        assert isinstance(got, tuple) and len(got) == len(want) and all(g is w for g, w in zip(got, want))


def test_the_table_cache_uploads_once_per_name_and_device_and_is_the_front_ends_too():
    dummy, cpu = Dummy("rows"), torch.device("cpu")
    t = dummy.table_on(cpu)
    assert t.dtype == torch.float32 and t.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert dummy.table_on(cpu) is t and dummy.table_on("cpu") is t and dummy.table_on(cpu, "table") is t
    other = dummy.table_on(cpu, "other")
    assert other is not t and other.shape == (5,) and dummy.table_on(cpu, "other") is other and dummy.table_on(cpu) is t
    both = dummy.table_on(cpu, ("table", "other"))
    assert isinstance(both, tuple) and [tuple(b.shape) for b in both] == [(4,), (5,)] and dummy.table_on(cpu, ("table", "other")) is both
    assert Dummy("rows").table_on(cpu) is not t                             # per object
    assert FrontEnd.table_on is DeviceTables.table_on is Stage.table_on and issubclass(FrontEnd, DeviceTables)
    from vit_vs_raw_iq_amd import Receiver
    for cls in (Receiver, Carrier, LikelihoodClassifier, Equaliser):
        assert cls.table_on is DeviceTables.table_on
    cr = Carrier(32, n_dft=(32, 32))
    t1, t2, tw = cr.tables_on(cpu)
    assert cr.tables_on(cpu)[0] is t1 and (t1.shape, t2.shape, tw.shape) == ((2, 32, 32), (2, 32, 32), (2, 1024))
    clf = LikelihoodClassifier(8, classes=["BPSK", "QPSK"], rotations=4)
    points, rot = clf.tables_on(cpu)
    assert clf.tables_on(cpu)[1] is rot and (points.shape, rot.shape) == ((6, 2), (4, 2))
    rx = Receiver(2, span=1, n_frac=1, timing="energy")
    assert rx.table_on(cpu) is rx.table_on(cpu) and np.array_equal(rx.table_on(cpu).numpy(), rx.table)


STAGES = {"carrier": (Carrier, lambda layout: Carrier(32, n_dft=(32, 32), layout=layout), ("interleaved", "planar"), "planar",
                      "carrier_reference"),
          "equaliser": (Equaliser, lambda layout: Equaliser(32, layout=layout), ("frames", "planar"), "frames",
                        "equaliser_reference"),
          "likelihood": (LikelihoodClassifier, lambda layout: LikelihoodClassifier(32, classes=["BPSK"], rotations=1, layout=layout),
                         ("frames", "planar"), "frames", "likelihood_reference")}


@pytest.mark.parametrize("name", list(STAGES))
def test_the_stages_derive_from_the_base_under_their_own_layout_names(name):
    import importlib
    cls, make, layouts, default, reference = STAGES[name]
    assert issubclass(cls, Stage) and cls.LAYOUTS == layouts and cls.reference == reference
    assert importlib.import_module("vit_vs_raw_iq_amd." + name).LAYOUTS == layouts
    for layout, shape in zip(layouts, ((5, 32, 2), (5, 2, 32))):
        stage = make(layout)
        assert stage.frame_shape(5) == shape and stage.layout == layout and stage.planar == layouts.index(layout) and stage.length == 32
    assert cls(32).layout == default
    for alias in set(("interleaved", "frames", "rows")) - set(layouts):
        with pytest.raises(ValueError, match="layout must be one of"):
            make(alias)


def test_stage_for_refuses_in_the_callers_words():
    eq = Equaliser(32, layout="planar")
    args = (Equaliser, "equaliser", True, 32, "the front ends read planar (B, 2, length) frames", "samples, the front end for 32")
    assert stage_for(eq, *args) is eq and stage_for(None, *args) is None
    with pytest.raises(TypeError, match="equaliser must be an Equaliser or None, got int"):
        stage_for(3, *args)
    with pytest.raises(TypeError, match="carrier must be a Carrier, got NoneType"):
        stage_for(None, Carrier, "carrier", True, 32, "", "", optional=False)
    with pytest.raises(ValueError, match=r"the front ends read planar \(B, 2, length\) frames: the equaliser's layout is 'frames'"):
        stage_for(Equaliser(32), *args)
    with pytest.raises(ValueError, match="the equaliser was built for frames of 31 samples, the front end for 32"):
        stage_for(Equaliser(31, layout="planar"), *args)
    with pytest.raises(ValueError, match=r"the receiver writes \(B, length, 2\) frames: the equaliser's layout is 'planar'"):
        stage_for(eq, Equaliser, "equaliser", False, 32, "the receiver writes (B, length, 2) frames", "symbols, the receiver gives 32")


MODULES = ["receiver", "carrier", "equaliser", "likelihood", "frontend", "synth", "waveform"]
# the package as a bare namespace, so that the module under test is the FIRST of the package to be imported (the package's
# __init__ would import every module in its own order and hide an import cycle), then the package itself
CHILD = """import importlib, os, sys, types
pkg = types.ModuleType('vit_vs_raw_iq_amd')
pkg.__path__ = [os.path.join(os.getcwd(), 'vit-vs-raw-iq_amd')]
sys.modules['vit_vs_raw_iq_amd'] = pkg
importlib.import_module('vit_vs_raw_iq_amd.{module}')
import vit_vs_raw_iq_amd.stage as S, vit_vs_raw_iq_amd._args as A
for name, m in sys.modules.items():
    if name.startswith('vit_vs_raw_iq_amd.') and name != 'vit_vs_raw_iq_amd.data':
        assert getattr(m, 'MAX_LENGTH', A.MAX_LENGTH) is A.MAX_LENGTH and getattr(m, '_host', S._host) is S._host, name
        assert getattr(m, '_frames', S._frames) is S._frames and getattr(m, '_first_largest', S._first_largest) is S._first_largest
del sys.modules['vit_vs_raw_iq_amd']
import vit_vs_raw_iq_amd
"""


def test_the_shared_module_imports_nothing_of_the_package_but_native_and_args():
    import ast
    import vit_vs_raw_iq_amd.stage as S
    tree = ast.parse(open(S.__file__).read())
    local = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level > 0]
    assert sorted(a.name if n.module is None else n.module for n in local for a in n.names[:1]) == ["_args", "_native"]
    assert not any(isinstance(n, ast.Import) and any(a.name.startswith("vit_vs") for a in n.names) for n in ast.walk(tree))


@pytest.fixture(scope="module")
def children():
    """One fresh interpreter per module, all started at once (`-c` puts the working directory on sys.path)."""
    procs = {m: subprocess.Popen([sys.executable, "-c", CHILD.format(module=m)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                 text=True, cwd=ROOT) for m in MODULES}
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()


@pytest.mark.parametrize("module", MODULES)
def test_each_module_imports_alone_in_a_fresh_interpreter(module, children):
    _, err = children[module].communicate()
    assert children[module].returncode == 0, err
