"""The table of tests/ctx_poison_cases.py against the sources (no device): every call site of slam_workspace, slam_io_arena and
radius_tables is run through by a case, every case names a reference that exists and masks only what the header leaves
undefined, and the hook slam_ctx_block_fill is in the ABI and refuses without a device."""
import collections
import importlib
import os
import re

import pytest

import ctx_poison_cases as T

CALL = re.compile(r"\b(slam_workspace|slam_io_arena|radius_tables)\(ctx\b")
HEAD = re.compile(r"^[A-Za-z_][^;{}]*?\b(\w+)\(")


def call_sites():
    """{file: [(callee, enclosing function), ...]} over csrc; the declarations of internal.h and the definitions take
    ``slam_ctx* ctx`` and are not call sites."""
    sites = {}
    for name in sorted(os.listdir(T.CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        fn = None
        for line in open(os.path.join(T.CSRC, name)):
            head = HEAD.match(line)
            if head and not line.rstrip().endswith(";") and not line.startswith(("//", "#")):
                fn = head.group(1)
            for m in CALL.finditer(line.split("//")[0]):
                sites.setdefault(name, []).append((m.group(1), fn))
    return sites


def test_every_call_site_has_its_case_and_every_case_its_call_site():
    sites = call_sites()
    listed = {}
    for c in T.CASES:
        assert os.path.exists(os.path.join(T.CSRC, c.file)), c.name
        for s in c.sites:
            listed.setdefault(c.file, []).append(s)
    for f in sorted(set(sites) | set(listed)):
        assert collections.Counter(sites.get(f, [])) == collections.Counter(listed.get(f, [])), \
            f"{f}: call sites {sorted(sites.get(f, []))} but the table covers {sorted(listed.get(f, []))}"
    ws = {f: [s for s in v if s[0] == "slam_workspace"] for f, v in sites.items()}
    ws = {f: v for f, v in ws.items() if v}
    assert (sum(len(v) for v in ws.values()), len(ws)) == (21, 16), {f: len(v) for f, v in ws.items()}
    per_file = {f: len(v) for f, v in ws.items()}
    assert {f for f, n in per_file.items() if n == 2} == {"proj_match.hip", "bow_match.hip", "tri_match.hip", "fuse.hip", "graph_lm.h"}
    # a file's entry points with a call site have at least as many cases as the file has call sites in distinct functions
    for f, v in sites.items():
        assert len([c for c in T.CASES if c.file == f and c.sites]) >= len({fn for _, fn in v}), f


def test_a_case_removed_from_the_table_fails_the_count(monkeypatch):
    monkeypatch.setattr(T, "CASES", [c for c in T.CASES if c.name != "pnp-ransac"])
    with pytest.raises(AssertionError, match="pnp.hip"):
        test_every_call_site_has_its_case_and_every_case_its_call_site()


def test_every_case_names_its_entry_point_and_a_reference_that_exists():
    header = open(T.HEADER).read()
    assert len({c.name for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert re.search(r"SLAM_API int %s\(" % c.entry, header), (c.name, c.entry)
        src = open(os.path.join(T.CSRC, c.file)).read()
        if c.file != "graph_lm.h":                               # (the graph entry points are instantiated in pose_graph.hip / sim3_graph.hip)
            assert re.search(r'extern "C" int %s\(' % c.entry, src), (c.name, c.entry)
        module, attr = c.reference.split(":")
        assert callable(getattr(importlib.import_module(module), attr)), (c.name, c.reference)
        assert callable(c._build)


UNDEFINED = []          # (case, output): the elements a header leaves undefined; no case of the table returns one today


def test_masks_are_the_listed_undefined_elements_and_quote_the_header():
    header = " ".join(open(T.HEADER).read().split())
    got = [(c.name, name) for c in T.CASES for name, _where, _line in c.undefined]
    assert sorted(got) == sorted(UNDEFINED)
    for c in T.CASES:
        for name, where, line in c.undefined:
            assert callable(where) and " ".join(line.split()) in header, (c.name, name, line)


def test_the_required_shapes_are_in_the_table():
    names = {c.name for c in T.CASES}
    for family in ("two-view", "homography", "pnp", "sim3"):
        assert f"{family}-ransac" in names
    for m in ("proj", "bow", "tri"):
        assert {f"{m}-search-tables", f"{m}-search-own-tables"} <= names
    assert {"fuse-search-tables", "fuse-search-no-tables", "fuse-refresh", "proj-project", "proj-grid", "bow-group", "tri-triangulate"} <= names
    assert {"top2-chunks-valu", "top2-chunks-mx16", "top2-chunks-mx32", "radius-short", "radius-long-host", "radius-total-only"} <= names
    assert T.POISON_BYTES == (0x00, 0xFF, 0x7F)


# ---- the hook in the ABI ----------------------------------------------------------------------------------------------------
def test_hook_is_in_the_abi_table_and_refuses_without_a_device(built):
    import ctypes

    from slamhip import _lib

    assert _lib.SIGNATURES["slam_ctx_block_fill"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int])
    lib = _lib.load()
    assert "SLAM_API int slam_ctx_block_fill(slam_ctx* ctx, int block, int byte);" in open(T.HEADER).read()
    for block in (0, 1, 3, 6, -1):
        assert lib.slam_ctx_block_fill(None, block, 0xFF) == _lib.SLAM_ERR_INVALID == -1
        assert b"slam_ctx_block_fill" in lib.slam_last_error()
    from slamhip.device import Context
    assert Context.BLOCKS.index("workspace") == 0 and Context.BLOCKS.index("io_dev") == 3 and Context.BLOCKS.index("io_host") == 4
    assert Context.BLOCKS.index("radius_tables") == 5 and callable(Context.fill_block)
