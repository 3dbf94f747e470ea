"""tests/test_gpu_mlp_call.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_ingest.py runs its file): both kernels of csrc/gaussians.hip against the ray kernels' rows and the float64
oracle, MLP.__call__ against the composed model's ray_history, against the reference's MLP in bf16 and in fp32 mode, its
argument errors and the training state it must leave alone, with the test code unchanged (about two and a half minutes).
One test is left to the MI355X: `test_host_tensors_are_refused`, because the simulated device IS the host and the session
switches the "must be a device tensor" check off (tests/sim_helpers.py), so there is nothing for the call to refuse."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_mlp_call_passes_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_mlp_call.py', '-k', 'not host_tensors']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
