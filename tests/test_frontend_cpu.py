"""CPU: the protocol of the image front ends (vit_vs_raw_iq_amd.frontend) on a dummy subclass, the geometry names of the three
real classes, and that every module which uses a front end imports on its own."""
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from vit_vs_raw_iq_amd import Constellation, CyclicSpectrum, IqError, Spectrogram
from vit_vs_raw_iq_amd.frontend import FrontEnd, front_end


class Dummy(FrontEnd):
    height, width = 32, 64

    def __init__(self):
        super().__init__(100)

    def struct(self):
        return None


def test_front_end_returns_the_object_or_refuses_with_the_messages_the_input_paths_always_gave():
    dummy = Dummy()
    assert front_end(dummy, "vit", 100) is dummy and front_end(None, "rawiq", 100) is None
    with pytest.raises(TypeError, match="spectrogram must be a Spectrogram or None, got int"):
        front_end(3, "vit", 100)
    with pytest.raises(ValueError, match="a spectrogram is an image: layout must be 'vit', got 'rawiq'"):
        front_end(dummy, "rawiq", 100)
    with pytest.raises(ValueError, match="the spectrogram was built for frames of 100 samples, these have 101"):
        front_end(dummy, "vit", 101)


def test_check_refuses_a_wrong_shape_and_a_cpu_tensor():
    dummy = Dummy()
    for bad in (torch.zeros(2, 2, 99), torch.zeros(2, 3, 100), torch.zeros(2, 100), [[0.0] * 100] * 2):
        with pytest.raises(ValueError, match=r"x must be a \(B, 2, 100\) tensor"):
            dummy._check(bad)
    with pytest.raises(ValueError, match="x_subset must be"):
        dummy.fit(torch.zeros(2, 2, 99))
    with pytest.raises(IqError, match="Dummy runs on the MI355X only: x is a CPU tensor and there is no CPU fallback"):
        dummy._check(torch.zeros(2, 2, 100))
    with pytest.raises(IqError, match="no CPU fallback"):
        dummy(torch.zeros(0, 2, 100))


FRONTS = {"spectrogram": (lambda: Spectrogram(32, 64, 100), 100, (5, 1, 32, 64)),
          "cyclic_both": (lambda: CyclicSpectrum(64, 256, kind="both"), 256, (5, 2, 64, 64)),
          "cyclic_conj": (lambda: CyclicSpectrum(64, 256, kind="conj"), 256, (5, 1, 64, 64)),
          "constellation": (lambda: Constellation(32, 64, 24), 24, (5, 1, 32, 64)),
          "dummy": (Dummy, 100, (5, 1, 32, 64))}


@pytest.mark.parametrize("name", list(FRONTS))
def test_image_shape_is_the_documented_shape_under_one_set_of_names(name):
    make, length, shape = FRONTS[name]
    front = make()
    assert isinstance(front, FrontEnd) and front.image_shape(5) == shape
    assert (front.channels, front.height, front.width, front.length) == shape[1:] + (length,)
    if name != "dummy":
        assert front.n_fft == front.height


MODULES = ["spectrogram", "cyclic", "constellation", "impairments", "synth", "data"]
CHILD = """import sys, vit_vs_raw_iq_amd.{module}
import vit_vs_raw_iq_amd.frontend as F, vit_vs_raw_iq_amd.impairments as I
assert I.front_end is F.front_end and I._front_end is F.front_end
for n, c in (('spectrogram', 'Spectrogram'), ('cyclic', 'CyclicSpectrum'), ('constellation', 'Constellation')):
    assert issubclass(getattr(sys.modules['vit_vs_raw_iq_amd.' + n], c), F.FrontEnd)
"""


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
def test_each_module_imports_alone_with_the_front_ends_bound_at_import(module, children):
    _, err = children[module].communicate()
    assert children[module].returncode == 0, err
