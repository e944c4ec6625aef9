"""CPU: the tables of tests/call_order_cases.py against include/qmps_hip.h - no GPU, no library call.

A new entry point cannot be added without taking its place: every `qmps_*` function the header declares is called by a family, a reader
or the settings probe of the call-order tests, or stands in NOT_STATEFUL.  EXPECT answers every (family, reader) pair with one of the
three outcomes and the header sentence it rests on; the list of families exempt from byte identity is frozen; the inputs are
reproducible."""
import os
import re

import numpy as np
import pytest

import call_order_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'qmps_hip.h')).read()


def test_every_entry_point_has_its_place():
    declared = set(C.declared_entry_points(HEADER))
    assert len(declared) > 80 and {'qmps_create', 'qmps_last_error', 'qmps_energy_launch', 'qmps_bw_env'} <= declared      # (the parser sees both return types)
    from qmps_amd import _lib
    assert declared == set(_lib.SIGNATURES), sorted(declared ^ set(_lib.SIGNATURES))
    called = C.called_entry_points()
    assert not (called | C.NOT_STATEFUL) - declared, sorted((called | C.NOT_STATEFUL) - declared)
    assert not called & C.NOT_STATEFUL - {'qmps_evolve_opts_init'}, sorted(called & C.NOT_STATEFUL)       # (the options helper fills a struct on the way)
    missing = declared - called - C.NOT_STATEFUL
    assert not missing, f'no family, reader or probe of tests/call_order_cases.py calls {sorted(missing)}: add one, or list it in NOT_STATEFUL with its reason'


def test_not_stateful_is_what_its_comment_says():
    allowed = re.compile(r'qmps_(abi_|last_error|selftest_|device_|timer_|kernel_time|set_kernel_timing_period|probe_|comm_|allreduce_|exchange_stats|evolve_opts_init)')
    assert all(allowed.match(name) for name in C.NOT_STATEFUL), sorted(n for n in C.NOT_STATEFUL if not allowed.match(n))


def test_expect_answers_every_pair():
    outcomes = {'same', 'of X', 'refuse'}
    for name, fam in C.FAMILIES.items():
        assert fam.Ds and set(fam.Ds) <= set(C.DS)
        for D in fam.Ds:
            assert fam.leaves(D) in C.LEAVES, (name, D)
            for reader in C.READERS:
                outcome, sentence = C.EXPECT[(name, D, reader)]
                assert outcome in outcomes and len(sentence) > 40, (name, D, reader)
    assert len(C.EXPECT) == sum(len(f.Ds) for f in C.FAMILIES.values()) * len(C.READERS)
    assert set(C.READERS) == set(C.ENERGY_READERS) | set(C.OVERLAP_READERS) and len(C.READERS) == 14


def test_quoted_sentences_stand_in_the_header():
    """what EXPECT quotes between double quotes is the header's text (whitespace and comment stars aside)"""
    flat = re.sub(r'\s+', ' ', re.sub(r'\n\s*\*', ' ', HEADER))
    for key, sentence in C._S.items():
        for quote in re.findall(r'"([^"]+)"', sentence):
            for piece in quote.split(' ... '):
                assert re.sub(r'\s+', ' ', piece).strip() in flat, (key, piece)


def test_exempt_list_is_frozen():
    assert C.EXEMPT_FROM_BYTES == frozenset()
    assert C.EXEMPT_FROM_BYTES <= set(C.FAMILIES)


def test_capped_variants_and_shapes():
    assert (C.B, C.WINDOWS, C.N, C.R, C.T, C.P, C.CAPACITY) == (37, 3, 111, 5, 3, 4, 256)
    assert 6 * C.R <= C.CAPACITY and C.T * (1 + 2 * C.P) <= C.CAPACITY and C.N <= C.CAPACITY      # double rotosolve, gradient batch, three windows
    assert C.B % 64 and C.B % 16 and C.B % 4                                                      # ragged last wave, tile and quad
    assert {f'energies_plain_cap{C.CAP_SHORT}', f'overlaps_tensor_r_cap{C.CAP_SHORT}', f'launch_krylov_cap{C.CAP_KRYLOV}',
            f'energies_slow_cap{C.CAP_KRYLOV}', f'overlaps_far_cap{C.CAP_KRYLOV}'} <= set(C.CAPPED)
    for name in C.CAPPED:
        if name.endswith(f'_cap{C.CAP_KRYLOV}'):
            assert C.FAMILIES[name].Ds == (8, 16), name
    assert C.CAP_KRYLOV > 64          # "Not ... with max_iter <= 64": below it nothing is handed to the fall-back
    h = C.inputs(4)['h']
    assert h.shape == (2, 4, 4) and np.abs(h[0] - h[0].conj().T).max() == 0 and np.abs(h[1] - h[1].conj().T).max() > 0.1


@pytest.mark.parametrize('D', C.DS)
def test_inputs_are_reproducible(D):
    a, b = C.build_inputs(D), C.build_inputs(D)
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert not a[k].flags.writeable
    if D == 16:
        from batch_edge_cases import pending_pool
        assert np.array_equal(a['slow'], pending_pool()[:C.B])


def test_every_family_names_the_settings_it_replaces():
    for name in C.FAMILIES:
        assert C.replaced_settings(name) <= set(C.SETTINGS), name
    assert 'hamiltonian' in C.replaced_settings('energies_direct') and 'overlap' in C.replaced_settings('evolve_bfgs')
    assert not C.replaced_settings('ansatz_probe') and not C.replaced_settings('bw_env')
