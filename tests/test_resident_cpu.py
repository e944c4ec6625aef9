"""CPU: qmps_amd/csrc/qmps_resident.h (qmps_slots, ResidentStates) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program: tests/csrc/resident_check.cpp, built on first use and run as a child process - nothing is loaded into Python."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'csrc')
HEADER = os.path.join(ROOT, 'qmps_amd', 'csrc', 'qmps_resident.h')
# the sanitizer runtimes are linked statically: the program carries them itself, whatever else the environment preloads
FLAGS = ['-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
         '-static-libasan', '-static-libubsan']


@functools.lru_cache(maxsize=None)
def checker():
    """tests/csrc/resident_check, rebuilt when its source, the header or this file (the flags) is newer"""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = os.path.join(HERE, 'resident_check.cpp'), os.path.join(HERE, 'resident_check')
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, HEADER, os.path.abspath(__file__))):
        subprocess.check_call([cxx] + FLAGS + ['-I', os.path.dirname(HEADER), '-o', exe + '.tmp', src], cwd=HERE)
        os.replace(exe + '.tmp', exe)
    return exe


def test_the_header_is_free_of_hip_and_compiles_alone():
    text = open(HEADER).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith('#include')]
    assert sorted(includes) == ['<stdint.h>', '<utility>', '<vector>'], includes
    subprocess.run([os.environ.get('CXX', 'g++'), '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-I', os.path.dirname(HEADER), '-x', 'c++', '-'],
                   input='#include "qmps_resident.h"\nint main() { return 0; }\n', text=True, check=True)


def test_slots_and_resident_states_against_their_models_under_the_sanitizers():
    """qmps_slots against a bitmap model over 2 000 x 40 random operations (invariant and union after each, touches / covers on proper,
    empty and inverted ranges); every ResidentStates transition from every reachable state.  The program prints what it compared."""
    def run_checker(**options):
        return subprocess.run([checker()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **options), timeout=300)
    run = run_checker()
    print(run.stdout)
    if run.returncode != 0 and 'LeakSanitizer has encountered a fatal error' in run.stdout and 'FAILED' not in run.stdout:
        # the leak pass at exit attaches to the process with ptrace; where the machine does not let it, everything but that pass runs
        run = run_checker(ASAN_OPTIONS='detect_leaks=0')
        print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    assert 'qmps_slots: 2000 sequences x 40 operations' in run.stdout and 'ResidentStates:' in run.stdout
    assert 'agree with the model' in run.stdout and 'every field as stated' in run.stdout
