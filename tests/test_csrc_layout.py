"""CPU: source checks of qmps_amd/csrc - the library is built from exactly the translation units that are there, and every small
device helper has one definition."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'qmps_amd', 'csrc')

SHARED_HELPERS = ('cmul', 'cmulc', 'cfma', 'cfms', 'cfma_conj', 'cfma_cj', 'cmma16', 'cmma16_3m', 'swz32', 'rx_lanes', 'crecip',
                  # the wave-level steps of the 16 x 16 matrix-core solves (qmps_tile16.h)
                  'tile16_to_a_layout', 'tile16_at', 'tile16_publish', 'tile16_fetch', 'tile16_merge_pair', 'tile16_mix_pairs',
                  'tile16_split_setup', 'tile16_cold_start', 'tile16_warm_start', 'tile16_power_test',
                  # the correlator sums: what every kernel shares (qmps_corrsum_core.h) and the helpers of the two sources
                  'pivot_size', 'pivot_usable', 'pair_products', 'left_products', 'matrix_entry', 'wave_argmax', 'row16_max', 'row16_sum16',
                  'op_dot', 'op_prod_dot', 'op2_dot', 'op2_prod_dot', 'cross_add')


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.hip')))
    assert len(files) > 30
    return {os.path.basename(f): open(f).read() for f in files}


def test_makefile_builds_exactly_the_translation_units_present():
    """SRCS is an explicit list (a stray scratch file never enters the library) and it names every *.hip file, once."""
    make = open(os.path.join(CSRC, 'Makefile')).read().replace('\\\n', ' ')
    srcs = re.search(r'^SRCS\s*:=\s*(.*)$', make, flags=re.M).group(1).split()
    assert len(srcs) == len(set(srcs))
    assert sorted(srcs) == sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, '*.hip')))
    assert 'wildcard' not in ' '.join(srcs)
    # every header is a dependency of every object: a new header cannot be a silently missing one
    rule = re.search(r'^build/%\.o:\s*(.*)$', make, flags=re.M).group(1)
    assert '$(wildcard *.h)' in rule and '../../include/qmps_hip.h' in rule
    assert not os.path.exists(os.path.join(CSRC, 'qmps_kernels.hip'))


def test_each_shared_device_helper_is_defined_once():
    src = sources()
    for name in SHARED_HELPERS:
        where = [f for f, text in src.items()
                 for _ in re.findall(r'__device__ __forceinline__ [\w:]+ %s\(' % re.escape(name), text)]
        assert len(where) == 1, f'{name}: defined in {where}'
    for f, text in src.items():
        # the names the copies used to hide behind
        assert 'cfma_conj1' not in text, f
        assert not re.search(r'\bcmma\(', text), f
        assert not re.search(r'\bswz<', text), f
        assert not re.search(r'\brx_cross\b', text), f
        assert 'auto to_a_layout' not in text, f


def test_the_overlap_dispatch_file_holds_no_kernels():
    """qmps_overlap.hip chooses the kernel family; the kernels live in one file per family."""
    src = sources()
    assert '__global__' not in src['qmps_overlap.hip']
    for f in ('qmps_overlap_block.hip', 'qmps_overlap_d16.hip', 'qmps_overlap_square.hip'):
        assert '__global__' in src[f], f


def test_the_overlap_switches_are_read_in_overlap_route_only():
    """The host code of the overlap side (objective, gradient, BFGS and rotosolve drivers) takes its kernel route from
    overlap_route(): outside that function the five switch names occur in comments only."""
    switches = ('QMPS_D16_BLOCK', 'QMPS_D16_ONE_WAVE', 'QMPS_NO_KRYLOV', 'QMPS_NO_DEFLATION', 'QMPS_OVERLAP_POWER')
    src = sources()
    text = src['qmps_capi_overlap.hip']
    start = text.index('OverlapRoute overlap_route(const qmps_ctx* c) {')
    end = text.index('\n}\n', start)
    route = text[start:end]
    for name in switches:
        assert 'documented_switch("%s")' % name in route, name
    executable = {'qmps_capi_overlap.hip': text[:start] + text[end:], 'qmps_capi_evolve.hip': src['qmps_capi_evolve.hip'],
                  'qmps_capi_roto.hip': src['qmps_capi_roto.hip']}
    for f, code in executable.items():
        assert '/*' not in code, f
        code = re.sub(r'//.*', '', code)
        for name in switches:
            assert name not in code, (f, name)
    assert 'overlap_squares' not in ''.join(src.values())


def test_the_correlator_sum_dispatch_file_holds_no_kernels_and_no_kernel_asks_for_the_source():
    """qmps_corrsum.hip checks the arguments and chooses the kernel family; the source of the right-hand sides is a type the kernels
    are instantiated with (OneSiteSource, TwoSiteSource), never a value they branch on."""
    src = sources()
    assert '__global__' not in src['qmps_corrsum.hip']
    for f in ('qmps_corrsum_small.hip', 'qmps_corrsum_block.hip'):
        assert '__global__' in src[f], f
    for f, text in src.items():
        for gone in ('Source::one_site', 'Source::two_site', 'if constexpr (SRC'):
            assert gone not in text, (f, gone)


STATE_FIELDS = ('count', 'has_tensors', 'ansatz', 'kind', 'P', 'rows', 'shift_index', 'shifts')


def test_the_resident_states_change_through_their_transitions_only():
    """ResidentStates (qmps_resident.h) is assigned by its own member functions; everything else reads `states.<field>`.  The loose
    fields it replaces are gone from the context and from the C-API files (LaneArgs, the launch argument of qmps_kernels.h, keeps
    its ans_i and ans_nsh: in the C-API files the two names occur as members of a LaneArgs `a` only).  The search knows the spelling
    `states.<field> =` alone: an assignment through a non-const reference to `states` would pass it, so the C-API takes none."""
    src = sources()
    header = src['qmps_resident.h']
    for field in STATE_FIELDS:
        assert re.search(r'\b%s\b' % field, header[header.index('struct ResidentStates'):]), field
    assign = re.compile(r'states\.(%s)\s*=[^=]' % '|'.join(STATE_FIELDS))
    for f, text in src.items():
        if f != 'qmps_resident.h':
            assert not assign.search(re.sub(r'//.*', '', text)), f
    for f, text in src.items():
        assert not re.search(r'(?<!const )ResidentStates\s*&', text), f
    searched = {f: text for f, text in src.items() if f.startswith('qmps_capi') or f == 'qmps_ctx.h'}
    assert len(searched) == 10, sorted(searched)
    for f, text in searched.items():
        for gone in ('ans_have', 'ans_src', 'tensors_valid', 'n_states'):
            assert gone not in text, (f, gone)
        for member in ('ans_i', 'ans_nsh'):
            uses = re.findall(r'(.{2})\b%s\b' % member, text)
            assert f != 'qmps_ctx.h' or not uses, (f, member)
            assert all(u == 'a.' for u in uses), (f, member, uses)


def test_device_buffers_are_freed_in_grow_and_at_the_end_only():
    """hipFree in the C-API: inside grow() (qmps_ctx.h), in qmps_destroy, in the peak probes and for the tuning build's d_prof."""
    src = sources()
    ctx = src['qmps_ctx.h']
    start = ctx.index('int grow(T*& buf, Cap& cap, Cap need, size_t bytes) {')
    assert ctx.count('hipFree(') == 1 and start < ctx.index('hipFree(') < ctx.index('\n}\n', start)
    capi = src['qmps_capi.hip']
    start = capi.index('int qmps_destroy(qmps_ctx* c) try {')
    end = capi.index('QMPS_API_CATCH', start)
    assert 'hipFree(' not in capi[:start] + capi[end:] and 'hipFree(' in capi[start:end]
    for f, text in src.items():
        if f.startswith('qmps_capi') and f not in ('qmps_capi.hip', 'qmps_capi_probe.hip'):
            frees = [line.strip() for line in text.splitlines() if 'hipFree(' in line]
            assert frees == (['HIP_TRY(hipFree(d_prof));'] if f == 'qmps_capi_evolve.hip' else []), (f, frees)
    assert sum(text.count('but only %lld states are resident') for text in src.values()) == 1
