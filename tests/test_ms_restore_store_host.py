"""The host side of the hand-over of restored witnesses to a store (nhip_ms_archive_restore_shape,
nhip_ms_store_append_restored), no GPU: the binding's prototypes and the ABI version, argument errors,
and tests/native/ms_restore_check.cpp, a stand-alone program built once plainly and once under ASan + UBSan (nothing
is preloaded and nothing runs on a GPU): the integer header the shape kernels run per lane against
ms_archive_restore_plan, and the new mirror commit against ms_store_append_plan + ms_store_append_commit."""
import ctypes
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ENTRY_POINTS = {"nhip_ms_archive_restore_shape": 6, "nhip_ms_store_append_restored": 8}


def test_abi_and_prototypes():
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    assert lib.nhip_abi_version() >= 3400
    for name, argc in ENTRY_POINTS.items():
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(NATIVE), "..", "include", "neptune_hip.h")).read()
    for name in ("WAVES", "SCAN_WIDTH", "CARRY_LANES"):
        assert f"#define NHIP_MS_RESTORE_{name} {getattr(L, 'MS_RESTORE_' + name)}\n" in hdr
    assert callable(MS.Archive.restore_shape)
    assert callable(MS.WitnessStore.append_restored) and callable(MS.WitnessStore.append_restored_membership_proofs)


def test_null_handles_are_argument_errors():
    import neptune_hip._lib as L
    lib = L.load()
    out = L.MsUpdated()
    assert lib.nhip_ms_archive_restore_shape(None, None, None, None, 0, ctypes.byref(out)) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_append_restored(None, None, None, None, None, None, 0, None) == L.NHIP_ERR_ARG


def test_handles_without_inputs_are_argument_errors():
    import neptune_hip as nh
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    try:
        ctx = nh.Context(0)
    except nh.NhipError:
        pytest.skip("creating a context needs a device")
    with ctx, MS.WitnessStore(ctx) as store, MS.Archive(ctx) as archive:
        lib = ctx.lib
        assert lib.nhip_ms_store_append_restored(store._h, None, None, None, None, None, 0, None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_append_restored(None, archive._h, None, None, None, None, 0, None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_append_restored(store._h, archive._h, None, None, None, None, 3, None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_archive_restore_shape(archive._h, None, None, None, 3, ctypes.byref(L.MsUpdated())) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_archive_restore_shape(archive._h, None, None, None, 0, None) == L.NHIP_ERR_ARG
        assert store.counts() == (0, 0, 0, 0, 0)


def test_integer_header_and_mirror_commit_plain_and_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_restore.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in ("ms_restore_check", "ms_restore_check_san"):
        r = subprocess.run([os.path.join(tmp_path, exe)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-4000:])
        checks, failures = (int(x) for x in r.stdout.split()[1::2])
        assert checks >= 5000 and failures == 0, (exe, r.stdout)
