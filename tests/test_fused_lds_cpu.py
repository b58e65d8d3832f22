"""csrc/fused_lds.h, the LDS layouts the fused teacher kernels and their launchers both read: a stand-alone host program
(tests/native/fused_lds_host.cpp) compares bytes() with the launchers' earlier formulas over every shape of the kernels' domains."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'fast-human-pose-estimation.pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'fused_lds_host.cpp')


def test_lds_bytes_of_the_fused_teacher_kernels_are_the_launchers_earlier_formulas(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler for tests/native/fused_lds_host.cpp')
    exe = str(tmp_path / 'fused_lds_host')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + CSRC, SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0 and b'shapes ok' in r.stdout, r.stdout.decode()
