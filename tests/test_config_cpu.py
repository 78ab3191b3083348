"""The library's environment variables (cora_amd/csrc/config.h) without a GPU: the table behind cora_debug_config, the
list users read in include/cora_hip.h, and the names tests and tools set must agree; flags, per-call and once-per-process
entries behave as documented."""
import glob
import os
import re
import subprocess
import sys

from cora_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"\bCORA_[A-Z0-9_]*[A-Z0-9]\b")
# names the Python side reads (bench, build, loader, lock-step tracing) and tools/plan_sweep.sh's baseline label
PYTHON_SIDE = {"CORA_BUILD_JOBS", "CORA_LIB_VARIANT", "CORA_LOCKSTEP_TRACE", "CORA_VARIANT", "CORA_REBUILD_UNITS",
               "CORA_EXTRA_HIPCC_FLAGS", "CORA_DUMMY"}

# Runs in a fresh process (the once-per-process entries must not have been read yet): prints the config after each step.
CHILD = r"""
import ctypes, os, sys
lib = ctypes.CDLL(sys.argv[1])
def show():
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.cora_debug_config(buf, len(buf))
    assert 0 < n < len(buf)
    print(buf.value.decode().replace("\n", "|"))
show()
os.environ["CORA_STPCG_BATCH"] = "3"
os.environ["CORA_KAPPA_FOLD_MAX"] = "7"
show()
"""


def _config(env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("CORA_")}
    e.update(env)
    capi.load()  # (built when stale)
    out = subprocess.run([sys.executable, "-c", CHILD, build.LIB], env=e, check=True, stdout=subprocess.PIPE,
                         universal_newlines=True).stdout.split("\n")
    steps = [line for line in out if line.startswith("CORA_")]
    assert len(steps) == 2, out
    return [dict(item.split("=", 1) for item in s.split("|") if item) for s in steps]


def _table_names():
    return set(_config({})[0])


def _header_names():
    hdr = open(os.path.join(ROOT, "include", "cora_hip.h")).read()
    begin = hdr.index("/* EVERY environment variable the library reads")
    return set(NAME.findall(hdr[begin:hdr.index("*/", begin)]))


def test_header_lists_exactly_the_table():
    table, header = _table_names(), _header_names()
    assert table == header, ("in the table only: %s, in the header only: %s" % (sorted(table - header), sorted(header - table)))


def test_names_set_by_tests_and_tools_are_in_the_table():
    used = set()
    files = glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "tools", "*"))
    for f in files:
        if os.path.isfile(f) and os.path.basename(f) != os.path.basename(__file__):
            used |= set(NAME.findall(open(f, errors="replace").read()))
    # C constants of the public header and compile-time macros of the sources are not environment variables
    not_env = set(PYTHON_SIDE)
    hdr = open(os.path.join(ROOT, "include", "cora_hip.h")).read()
    not_env |= set(re.findall(r"#define\s+(CORA_[A-Z0-9_]+)", hdr)) | set(re.findall(r"\b(CORA_[A-Z0-9_]+)\s*=\s*-?\d", hdr))
    for f in glob.glob(os.path.join(ROOT, "cora_amd", "csrc", "**", "*"), recursive=True) + files:
        if os.path.isfile(f):
            not_env |= set(re.findall(r"(?:#\s*(?:if|ifdef|ifndef|elif|define)\s+!?\s*(?:defined\s*\(?\s*)?|-D)(CORA_[A-Z0-9_]+)",
                                      open(f, errors="replace").read()))
    missing = {n for n in used - not_env if not n.startswith("CORA_BENCH_")} - _table_names()
    assert not missing, "set by tests or tools but not read by the library: %s" % sorted(missing)


def test_flag_rule_and_lifetimes():
    on, _ = _config({"CORA_NO_FUSE": "1"})
    off, _ = _config({"CORA_NO_FUSE": "0"})
    unset, later = _config({})
    assert on["CORA_NO_FUSE"] == "1" and off["CORA_NO_FUSE"] == "0" and unset["CORA_NO_FUSE"] == "0 (default)"
    assert _config({"CORA_CHAIN_SLICES": "0"})[0]["CORA_CHAIN_SLICES"] == "0"
    assert unset["CORA_CHAIN_SLICES"] == "1 (default)"
    # per call: follows a later setenv; once per process: keeps the value of its first read
    assert unset["CORA_STPCG_BATCH"] == "0 (default)" and later["CORA_STPCG_BATCH"] == "3"
    assert unset["CORA_KAPPA_FOLD_MAX"] == "4096 (default)" and later["CORA_KAPPA_FOLD_MAX"] == "4096 (default)"
    # numbers keep their clamps
    clamped = _config({"CORA_TRI_SN_CAP": "99", "CORA_ND_LEAF": "0", "CORA_P2P_TIMEOUT_S": "0"})[0]
    assert clamped["CORA_TRI_SN_CAP"] == "32" and clamped["CORA_ND_LEAF"] == "1"
    assert float(clamped["CORA_P2P_TIMEOUT_S"]) == 0.001
