"""Who owns the solver's device buffers, pinned buffers, streams and events (the four owners of csrc/gar_host.hpp):
tests/cpp/test_lifetime.cpp drives the C ABI through create / lazy first uses / rebuild / refusal / destroy sequences,
linked against an emulator build of the library, both compiled with the host's AddressSanitizer (`make -C tests/cpp
asan`; the program links the sanitizer's runtime itself, nothing is preloaded).  On the emulator a device buffer, an
event and a stream are malloc blocks: a missed release is a leak report at exit, a double release or a use after a
rebuild an immediate error; the program also compares the allocation count of every scenario with the counts recorded
on the commit before the owners existed.  CPU only.  The sanitized emulator build takes about as long as the two
extra emulator builds of test_ldl_blocked.py together and is reused while it is up to date."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def test_lifetime_scenarios_under_the_host_sanitizer():
    subprocess.run(["make", "-s", "-C", CPP, "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CPP, "_build", "test_lifetime_asan")], capture_output=True, text=True, env=env,
                       timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lifetime ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "Sanitizer" not in r.stdout, r.stderr
