"""The route ledger (stablekeypoints_amd/routes.py) without a GPU: the ledger itself, the policy context managers, thread safety,
the host branches' notes, and static checks that every fall-through of the gated sites notes its route."""
import ast
import os
import re
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stablekeypoints_amd")


@pytest.fixture
def routes():
    from stablekeypoints_amd import routes as r
    r.reset()
    yield r
    r.reset()


def test_note_snapshot_reset_table(routes):
    assert routes.snapshot() == {} and routes.table() == "(no routes noted)"
    routes.note("conv3x3", "wino4_c128")
    routes.note("conv3x3", "wino4_c128", 2)
    routes.note("conv3x3", "lib")
    routes.note("resnet", "eager")
    routes.note("flash.fwd", "flash_split", 5)
    assert routes.snapshot() == {("conv3x3", "wino4_c128"): 3, ("conv3x3", "lib"): 1, ("resnet", "eager"): 1,
                                 ("flash.fwd", "flash_split"): 5}
    lines = routes.table().splitlines()
    head = lines[0].split()
    assert head[0] == "site" and "wino4_c128" in head and "lib[library]" in head and "eager[eager]" in head and "flash_split" in head
    rows = {ln.split()[0]: ln.split()[1:] for ln in lines[1:]}
    assert set(rows) == {"conv3x3", "resnet", "flash.fwd"}
    assert rows["conv3x3"][head.index("wino4_c128") - 1] == "3" and rows["conv3x3"][head.index("lib[library]") - 1] == "1"
    assert rows["resnet"][head.index("eager[eager]") - 1] == "1" and rows["resnet"][head.index("wino4_c128") - 1] == "."
    assert [(s, r, c, k) for s, r, c, k, _ in routes.non_hip()] == [("conv3x3", "lib", 1, "library"), ("resnet", "eager", 1, "eager")]
    for site, route in (("conv3x3", "wino4_c129"), ("conv4x4", "lib"), ("resnet", "lib")):
        with pytest.raises(KeyError):
            routes.note(site, route)
    assert routes.snapshot()[("conv3x3", "wino4_c128")] == 3                 # a refused note counts nothing
    before = routes.snapshot()
    routes.note("resnet", "fused", 4)
    d = routes.delta(before)
    assert d == {("resnet", "fused"): 4}
    routes.merge(d, 2)
    assert routes.snapshot()[("resnet", "fused")] == 12
    routes.merge(d, -3)
    assert ("resnet", "fused") not in routes.snapshot()
    routes.reset()
    assert routes.snapshot() == {}


def test_every_route_has_a_kind_and_documented_routes_are_registered(routes):
    assert routes.ROUTES
    for site, rs in routes.ROUTES.items():
        assert rs, site
        for route, kind in rs.items():
            assert kind in routes.KINDS, (site, route, kind)
            assert routes.kind(site, route) == kind
    for (site, route), reason in routes.DOCUMENTED_LIBRARY_ROUTES.items():
        assert routes.ROUTES[site][route] in ("library", "eager"), (site, route)
        assert isinstance(reason, str) and len(reason) > 20
    assert ("conv3x3", "lib") not in routes.DOCUMENTED_LIBRARY_ROUTES        # a Winograd-shaped layer on the library is a regression
    for name in ("eager", "host"):                                            # a route's name says its kind where the name is a kind
        for site, rs in routes.ROUTES.items():
            if name in rs:
                assert rs[name] == name


def test_expect_allow_and_strict(routes):
    with routes.expect():
        routes.note("conv3x3", "wino4_raw")
        routes.note("flash.bwd", "flash_f32", 3)
    routes.note("conv3x3", "lib", 7)                                          # noted before the block: not the block's business
    with pytest.raises(routes.UnexpectedRoute) as err:
        with routes.expect():
            routes.note("conv3x3", "wino2")
            routes.note("conv3x3", "lib", 2)
            routes.note("downsample", "eager")
            routes.note("attn.self", "host")
    assert err.value.found == [("attn.self", "host", 1), ("conv3x3", "lib", 2), ("downsample", "eager", 1)]
    assert "conv3x3/lib x2" in str(err.value) and "downsample/eager x1" in str(err.value)
    with pytest.raises(routes.UnexpectedRoute) as err:
        with routes.expect(allow=[("conv3x3", "lib"), ("attn.self", "host")]):
            routes.note("conv3x3", "lib")
            routes.note("conv3x3.bwd_data", "lib")                            # allow names pairs, not routes
            routes.note("attn.self", "host")
    assert err.value.found == [("conv3x3.bwd_data", "lib", 1)]
    with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES):               # the dict's keys are the pairs
        routes.note("vae.attention", "lib_core")
    with routes.expect(kinds=("hip", "host")):
        routes.note("map.fwd", "host")
    with pytest.raises(ZeroDivisionError):                                    # the block's own error is not masked
        with routes.expect():
            routes.note("conv3x3", "lib")
            1 / 0
    with routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
        routes.note("conv3x3", "wino4_c64")
        routes.note("vae.attention", "lib_core")
        with pytest.raises(routes.UnexpectedRoute) as err:
            routes.note("conv3x3", "lib")
        assert err.value.found == [("conv3x3", "lib", 1)]
        assert err.traceback[-1].name == "note"                               # raised inside note(): the caller's frame is the gate
        with pytest.raises(KeyError):
            routes.note("conv3x3", "nope")
    routes.note("conv3x3", "lib")                                             # the rule ends with the block
    with pytest.raises(ValueError):
        routes.guard("loud")
    with routes.guard("strict"):
        assert routes.snapshot() == {}                                        # report / strict start from an empty ledger
        with pytest.raises(routes.UnexpectedRoute):
            routes.note("resnet", "eager")
    routes.note("resnet", "eager")
    with routes.guard("off"):
        assert routes.snapshot()[("resnet", "eager")] == 2


def test_two_threads_note_exactly(routes):
    n = 100_000

    def work(route):
        for _ in range(n):
            routes.note("conv3x3", "wino4_c128")
            routes.note("conv3x3", route)
    ts = [threading.Thread(target=work, args=(r,)) for r in ("wino4_raw", "wino2")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert routes.snapshot() == {("conv3x3", "wino4_c128"): 2 * n, ("conv3x3", "wino4_raw"): n, ("conv3x3", "wino2"): n}


def test_host_branches_are_instrumented(routes):
    """The reduced-width tree on the CPU (the construction of tests/test_host_logic.py's `tiny_ldm`) through `run_and_find_attn` with
    a materialising store -- the only form of the map reduction that runs off the GPU: every route noted is a host route, and
    the attention cores, the per-layer map and the map reduction all appear."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=32)
    controllers[torch.device("cpu")].materialize = True
    routes.reset()
    with torch.no_grad():
        with routes.expect(kinds=("host",)):
            maps = ptp_utils.run_and_find_attn(ldm, torch.rand(1, 3, 128, 128), torch.randn(1, 9, 768), device="cpu",
                                               controllers=controllers, upsample_res=32)
    assert maps[0].shape == (9, 32, 32)
    snap = routes.snapshot()
    assert snap and all(routes.kind(s, r) == "host" for s, r in snap)
    assert snap[("attn.cross", "host")] > 0 and snap[("attn.self", "host")] > 0
    assert snap[("map.fwd", "host")] == 4 and snap[("map.collect", "host")] == 1


# ---------------------------------------------------------------------------------------------------------------------
# static checks
# ---------------------------------------------------------------------------------------------------------------------
def _is_note(stmt):
    return (isinstance(stmt, ast.Expr) and isinstance(stmt.value, ast.Call) and isinstance(stmt.value.func, ast.Attribute)
            and stmt.value.func.attr == "note" and isinstance(stmt.value.func.value, ast.Name) and stmt.value.func.value.id == "routes")


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
    return ".".join(reversed(parts))


def _note_route(stmt):
    """The route a `routes.note(site, route)` statement names, when it is a string literal (else "?")."""
    args = stmt.value.args
    return args[1].value if len(args) > 1 and isinstance(args[1], ast.Constant) and isinstance(args[1].value, str) else "?"


def _unnoted(func, is_target, want=("eager", "lib")):
    """Statements of `func` that satisfy `is_target` and are NOT preceded on their own path by a `routes.note(...)` statement whose
    route is one of `want`: the LAST note that is an earlier sibling of the statement, or of one of the blocks that enclose it,
    inside `func` -- the note that has necessarily run last when the target is reached -- must name a fall-through route, so a
    `fused` note at the top of a function does not cover a `return orig(...)` added further down.  -> [line numbers]."""
    missing = []

    def walk(body, noted):
        for stmt in body:
            if _is_note(stmt):
                noted = _note_route(stmt) in want
                continue
            if isinstance(stmt, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                continue                                                       # another scope: checked on its own
            if is_target(stmt) and not noted:
                missing.append(stmt.lineno)
            for field in ("body", "orelse", "finalbody"):
                walk(getattr(stmt, field, []) or [], noted)
            for h in getattr(stmt, "handlers", []) or []:
                walk(h.body, noted)
    walk(func.body, False)
    return missing


def _calls(stmt, pred):
    """Calls directly in `stmt` (not in nested compound bodies) that satisfy pred."""
    own = [stmt] if not hasattr(stmt, "body") else [getattr(stmt, "test", None), getattr(stmt, "iter", None)]
    return [n for root in own if root is not None for n in ast.walk(root) if isinstance(n, ast.Call) and pred(n)]


def _functions(tree):
    return [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def test_every_fall_through_notes_its_route():
    """`return orig(...)` in ldm/fused.py, and the library tails of `ops.conv3x3_auto`, `ops.Conv3x3Fn.backward` and
    `ops.ConvS2Fn.backward` (conv2d / conv2d_input calls), each come after a `routes.note(` on the same path."""
    src = open(os.path.join(PKG, "ldm", "fused.py")).read()
    tree = ast.parse(src)

    def returns_orig(stmt):
        return (isinstance(stmt, ast.Return) and isinstance(stmt.value, ast.Call) and isinstance(stmt.value.func, ast.Name)
                and stmt.value.func.id == "orig")
    n_returns = sum(1 for n in ast.walk(tree) if returns_orig(n))
    assert n_returns == len(re.findall(r"return orig\(", src)) and n_returns >= 8
    seen = 0
    for fn in _functions(tree):
        own = []
        bad = _unnoted(fn, lambda s: returns_orig(s) and not own.append(s.lineno))
        seen += len(own)
        assert not bad, f"ldm/fused.py: `return orig(...)` without a routes.note on its path, lines {bad}"
    assert seen == n_returns                                                  # every one was inside a checked function

    ops_tree = ast.parse(open(os.path.join(PKG, "ops.py")).read())
    LIB = {"torch.nn.functional.conv2d", "torch.nn.grad.conv2d_input", "F.conv2d"}

    def lib_call(stmt):
        return bool(_calls(stmt, lambda c: _dotted(c.func) in LIB))
    by_name = {}
    for node in ast.walk(ops_tree):
        if isinstance(node, ast.ClassDef):
            for f in node.body:
                if isinstance(f, ast.FunctionDef):
                    by_name[f"{node.name}.{f.name}"] = f
    for f in ops_tree.body:
        if isinstance(f, ast.FunctionDef):
            by_name[f.name] = f
    total = 0
    for name, want in (("conv3x3_auto", 2), ("Conv3x3Fn.backward", 1), ("ConvS2Fn.backward", 2)):
        fn = by_name[name]
        hits = []
        bad = _unnoted(fn, lambda s: lib_call(s) and not hits.append(s.lineno))
        assert len(hits) >= want, f"ops.{name}: expected at least {want} library convolution calls, found {len(hits)}"
        assert not bad, f"ops.{name}: library convolution without a routes.note on its path, lines {bad}"
        total += len(hits)
    # no other function of ops.py reaches the library convolutions
    everywhere = sum(1 for n in ast.walk(ops_tree) if isinstance(n, ast.Call) and _dotted(n.func) in LIB)
    assert everywhere == total


def test_static_check_itself_sees_a_missing_note():
    good = ast.parse("def f(x):\n    if x:\n        routes.note('a', 'b')\n        return orig(x)\n    routes.note('a', 'c')\n    return orig(x)\n").body[0]
    bad = ast.parse("def f(x):\n    if x:\n        routes.note('a', 'b')\n    else:\n        return orig(x)\n    return orig(x)\n").body[0]

    def returns_orig(s):
        return isinstance(s, ast.Return) and isinstance(s.value, ast.Call) and getattr(s.value.func, "id", "") == "orig"
    assert _unnoted(good, returns_orig, want=("b", "c")) == []
    assert _unnoted(bad, returns_orig, want=("b", "c")) == [5, 6]             # a note in a sibling branch does not count
    assert _unnoted(good, returns_orig, want=("c",)) == [4]                   # nor one that names another route
    late = ast.parse("def f(x):\n    routes.note('a', 'fused')\n    if x:\n        return orig(x)\n    return 1\n").body[0]
    assert _unnoted(late, returns_orig, want=("eager",)) == [4]


def test_routes_module_is_self_contained():
    """routes.py imports nothing from oracle/ (nor torch, nor the native library: `note()` cannot touch the device) and reads no
    environment variable."""
    src = open(os.path.join(PKG, "routes.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M)
    assert "environ" not in src and "getenv" not in src and not re.findall(r"[\"'](SKP_[A-Z0-9_]+)[\"']", src)
    imported = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            imported |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            imported.add((node.module or ".").split(".")[0] if node.level == 0 else ".")
    assert imported <= {"__future__", "contextlib", "functools", "threading", "typing"}, imported


def test_plan_names_follow_the_library(routes):
    """`routes.wino4_form` restates csrc/skp_conv_wino4.hip's wino4_use_c128: wherever the library's own query says the
    GroupNorm-folded kernel serves a launch (128-channel form, unsplit, <= 512 output channels) the name must be `wino4_c128`, and an
    unsplit launch of <= 512 output channels that the query refuses must be named `wino4_c64`."""
    from stablekeypoints_amd import _native as N
    lib = N.lib()
    checked, seen = 0, set()
    for rows in (1, 2, 4, 8, 16):
        for c in (64, 128, 192, 256, 320, 512):
            for side in (8, 16, 32, 64, 128, 256):
                if lib.skp_conv3x3_f4_workspace(rows, c, c, side, side) != 0:
                    continue                                                  # K-split launch: the query answers 0 for another reason
                want = "wino4_c128" if lib.skp_conv3x3_f4_gn_ok(rows, c, c, side, side) else "wino4_c64"
                assert routes.wino4_form(c, rows, side, side) == want, (rows, c, side)
                checked += 1
                seen.add(want)
    assert checked >= 20 and seen == {"wino4_c128", "wino4_c64"}, (checked, seen)
    # csrc/skp_cross_attn.hip's ca_use_ts, at the step's shapes: 16^2 x 1280 (d = 160) at 8 rows splits tokens, 64^2 x 320 (d = 40) never
    assert routes.cross_attn_form(8, 8, 256, 77, 160) == "ca_token_split" and routes.cross_attn_form(8, 8, 4096, 77, 40) == "ca_plain"
    assert routes.cross_attn_form(8, 8, 256, 77, 160, ts_off=True) == "ca_plain" and routes.cross_attn_form(8, 8, 256, 16, 160) == "ca_plain"
    assert routes.cross_attn_form(8, 8, 4096, 77, 80) == "ca_plain" and routes.cross_attn_form(2, 8, 1024, 77, 80) == "ca_token_split"


def test_routes_keyword_is_a_plain_parameter_and_its_rule_ends_with_the_call(routes):
    """The three entry points show `routes="off"` in their signature, refuse an unknown mode, and `routes="strict"` leaves no rule
    behind when the call fails early (here: a batch size the data-parallel width does not divide, raised before the loop)."""
    import inspect
    from types import SimpleNamespace
    from stablekeypoints_amd import eval as E, keypoint_regressor as K, optimize as O
    for fn in (O.optimize_embedding, K.precompute_all_keypoints, E.run_image_with_context_augmented):
        assert inspect.signature(fn).parameters["routes"].default == "off"
        assert "`routes`" in fn.__doc__
    with pytest.raises(ValueError, match="routes must be one of"):
        K.precompute_all_keypoints(None, None, None, None, None, 1, routes="loud")
    with pytest.raises(ValueError, match="routes must be one of"):
        E.run_image_with_context_augmented(None, None, None, None, routes="loud")
    with pytest.raises(ValueError, match="routes must be one of"):
        O.optimize_embedding(None, SimpleNamespace(batch_size=1), {}, 1, routes="loud")
    with pytest.raises(ValueError, match="batch_size"):
        O.optimize_embedding(None, SimpleNamespace(batch_size=0), {torch.device("cpu"): None}, 1, routes="strict")
    routes.note("conv3x3", "lib")                                             # no strict rule is left installed
    with pytest.raises(AttributeError):                                       # an error inside the inference entry points: the same
        K.precompute_all_keypoints(None, None, None, None, None, 1, routes="strict")
    routes.note("conv3x3", "lib")
    assert routes.snapshot() == {("conv3x3", "lib"): 1}                       # (strict started from an empty ledger)
