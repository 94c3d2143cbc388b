"""csrc/tdr_fft_core.h on the host: the header compiles without a device (TDR_FFT_HOST) and tests/fft_core_host.cpp runs every admissible
length, both plans (the split_tail plans of H = 640, 768, 1024 on the 8-column tile included, one of which fills MAX_STAGES) and both
line layouts against a naive double DFT, under the address and undefined-behaviour sanitizers where the compiler has them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fft_core_against_a_double_dft_on_the_host(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler on PATH')
    src, exe = os.path.join(ROOT, 'tests', 'fft_core_host.cpp'), str(tmp_path / 'fft_core_host')
    base = [cxx, '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'textualdegremoval_amd', 'csrc'), src, '-o', exe]
    if subprocess.run(base + ['-fsanitize=address,undefined'], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)                       # a compiler without the sanitizer runtimes
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'ok: 22 admissible lengths' in out.stdout
