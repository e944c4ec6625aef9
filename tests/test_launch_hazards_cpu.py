"""CPU: qmps_amd/csrc/qmps_hazard.h - which launches of the fused D = 4 energy kernel may overlap on the two launch lanes, and the waits
the context issues for those that may not - under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program:
tests/csrc/hazard_check.cpp, built on first use and run as a child process - nothing is loaded into Python."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'csrc')
HEADER = os.path.join(ROOT, 'qmps_amd', 'csrc', 'qmps_hazard.h')
# the sanitizer runtimes are linked statically: the program carries them itself, whatever else the environment preloads
FLAGS = ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
         '-static-libasan', '-static-libubsan']


@functools.lru_cache(maxsize=None)
def checker():
    """tests/csrc/hazard_check, rebuilt when its source, the header or this file (the flags) is newer"""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = os.path.join(HERE, 'hazard_check.cpp'), os.path.join(HERE, 'hazard_check')
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, HEADER, os.path.abspath(__file__))):
        subprocess.check_call([cxx] + FLAGS + ['-I', os.path.dirname(HEADER), '-o', exe + '.tmp', src], cwd=HERE)
        os.replace(exe + '.tmp', exe)
    return exe


def test_the_header_is_free_of_hip_and_compiles_alone():
    text = open(HEADER).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith('#include')]
    assert includes == ['<stdint.h>'], includes
    subprocess.run([os.environ.get('CXX', 'g++'), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-I', os.path.dirname(HEADER), '-x', 'c++', '-'],
                   input='#include "qmps_hazard.h"\nint main() { return 0; }\n', text=True, check=True)


def test_conflicts_and_waits_against_brute_force_under_the_sanitizers():
    """hazard_conflict against the read and write sets of every pair of 1 568 footprints over windows inside [0, 6); LaneTable with
    lanes_begin / lanes_join against a model of two in-order streams with events, over 400 random sequences of 300 operations: the
    same window every step, cycles of 3, 9 and 33 windows, windows at random, with and without other work in between.  The program
    prints what it compared."""
    def run_checker(**options):
        return subprocess.run([checker()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **options), timeout=300)
    run = run_checker()
    print(run.stdout)
    if run.returncode != 0 and 'LeakSanitizer has encountered a fatal error' in run.stdout and 'FAILED' not in run.stdout:
        # the leak pass at exit attaches to the process with ptrace; where the machine does not let it, everything but that pass runs
        run = run_checker(ASAN_OPTIONS='detect_leaks=0')
        print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert 'hazard_conflict: 1568 footprints' in run.stdout and 'agrees with brute force' in run.stdout
    assert 'LaneTable: 400 sequences x 300 operations' in run.stdout and 'every launch behind what it conflicts with' in run.stdout
