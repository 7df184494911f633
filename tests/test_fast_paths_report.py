"""model.fast_paths() - what bench.py prints as `host.fast_paths` - states the
paths a fresh process can take under each switch, none that is off.  No GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ('BNPC_NATIVE_MH', 'BNPC_NATIVE_BETA', 'BNPC_NATIVE_MOVES',
    'BNPC_NATIVE_STEP', 'BNPC_NATIVE_BIRTHS', 'BNPC_STREAM_LIVE',
    'BNPC_TIMING')
_KEYS = ['rng_live', 'gauss_live', 'scipy_capi', 'ufunc_loops', 'native_mh',
    'native_beta', 'native_moves', 'native_step']
_CHILD = ('import json, sys; sys.path.insert(0, %r); '
    'from bnpc_amd import model; print(json.dumps(model.fast_paths()))')


@pytest.mark.parametrize('switch,off', [
    (None, set()),
    ('BNPC_NATIVE_MH=0', {'native_mh', 'native_moves', 'native_step'}),
    ('BNPC_NATIVE_MOVES=0', {'native_moves', 'native_step'}),
    ('BNPC_NATIVE_STEP=0', {'native_step'}),
    ('BNPC_STREAM_LIVE=0', {'rng_live', 'gauss_live', 'native_step'}),
    ('BNPC_STREAM_LIVE=rng', {'gauss_live'}),
    ('BNPC_NATIVE_BIRTHS=0', set()),
    ('BNPC_TIMING=1', set()),
    # CRP._native_move makes no move without the native Beta sampler
    ('BNPC_NATIVE_BETA=0', {'native_beta', 'native_moves', 'native_step'})])
def test_report_of_a_fresh_process_under_each_switch(switch, off):
    """The keys in their order, and exactly the paths a switch turns off
    reported False."""
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    if switch:
        name, value = switch.split('=')
        env[name] = value
    out = subprocess.run([sys.executable, '-c', _CHILD % ROOT], env=env,
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    paths = json.loads(out.stdout.splitlines()[-1])
    assert list(paths) == _KEYS
    assert all(type(v) is bool for v in paths.values()), paths
    assert {k for k, v in paths.items() if not v} == off, paths
