"""CPU: the TypeScript-side host (bindings/ts/*.js + *.d.ts) covers the reference's operator surface -- pinned to reference-held DATA
(VERDICT r2 item 8).  ``tests/golden/reference_surface.json`` holds, per reference file, class -> public method -> (parameters, required
parameters), exported functions and interface members, extracted from the reference's sources by ``scripts/ts_surface.py --reference``
(names and arities only).  The same scanner reads this repo's CommonJS modules and typings; every entry must be there with the same arity, or be
listed in WAIVERS with the reason (INTEGRATION.md repeats the list).  The Python host is checked by name."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import ts_surface  # noqa: E402

# (class or interface, member) -> why it has no counterpart
WAIVERS = {
    ("PrefixScanner", "info_buffer"): "WebGPU plumbing: the uniform block carrying the element count; set_count() keeps the count, kernels take it as an argument (SURVEY 2.1 row 8: replaced)",
    ("PrefixScanner", "block_sums_buffer"): "internal scratch of the reference's 3-phase scan, 'exposed for debugging' (prefix.ts:35-36); the HIP scan owns its scratch",
    ("DynamicSortStuff", "sort_info_buffer"): "WebGPU plumbing: sort sizes derived on the GPU by update_dispatch (K7); the HIP sort reads the count from the stats buffer itself",
    ("DynamicSortStuff", "sort_dispatch_indirect_buffer"): "WebGPU plumbing: indirect-dispatch arguments (K7); HIP kernels are launched for the capacity and exit on the device-side count",
    ("DynamicSortStuff", "histogram_buffer"): "internal scratch of the reference's radix sort (K8-K10)",
    ("Trainer", "visualizeLoss"): "debug render pass that draws the loss texture on the canvas (trainer.ts:695-768): presentation, SURVEY 2.1 row 15; the image is TiledBackwardPass.getLossTextureView()",
}


JS_MODULES = ("webdgs_hip.js", "trainer.js", "viewer.js", "camera.js", "loaders.js", "images.js")


def _ours():
    js, dts = dict(classes={}, functions={}), dict(classes={}, functions={})
    for f in JS_MODULES:
        s = ts_surface.surface(open(os.path.join(ROOT, "bindings", "ts", f)).read())
        js["classes"].update(s["classes"]); js["functions"].update(s["functions"])
    for f in [m[:-3] + ".d.ts" for m in JS_MODULES]:
        s = ts_surface.surface(open(os.path.join(ROOT, "bindings", "ts", f)).read())
        dts["classes"].update(s["classes"]); dts["functions"].update(s["functions"])
    return js, dts


def _reference():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")))


def _declarations(f: dict) -> str:
    """TypeScript that declares exactly the surface of one fixture entry: exported classes with their public methods (the first `required`
    parameters required, the rest optional), exported interfaces, exported functions."""
    def params(n, required):
        return ", ".join(f"p{i}{'' if i < required else '?'}: number" for i in range(n))
    out = []
    for cname, methods in f["classes"].items():
        out.append(f"export class {cname} {{")
        for m, info in methods.items():
            prefix = ("static " if info["static"] else "") + {"getter": "get ", "setter": "set ", "method": ""}[info["kind"]]
            out.append(f"    {prefix}{m}({params(info['params'], info['required'])}) {{ }}")
        out.append("}")
    for iname, mem in f["interfaces"].items():
        out.append(f"export interface {iname} {{")
        out += [f"    {m}: number;" if n is None else f"    {m}: ({params(n, n)}) => void;" for m, n in mem.items()]
        out.append("}")
    out += [f"export function {fn}({params(info['params'], info['required'])}) {{ }}" for fn, info in f["functions"].items()]
    return "\n".join(out) + "\n"


def test_fixture_is_what_the_extractor_produces_from_the_surface_it_records(tmp_path):
    """The committed fixture is the extractor's own output: TypeScript declaring what it records, laid out under the reference's file names,
    extracted by ``ts_surface.reference_surface`` as the fixture was, gives the fixture back -- every file the extractor reads, no entry more
    or less, every arity and flag as the scanner counts it."""
    ref = _reference()
    for rel, f in ref["files"].items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(_declarations(f))
    assert sorted(ref["files"]) == sorted(ts_surface.REFERENCE_FILES)
    assert ts_surface.reference_surface(str(tmp_path)) == ref


def test_every_reference_class_method_exists_with_the_same_arity():
    ref, (js, dts) = _reference(), _ours()
    missing, checked = [], 0
    for rel, f in ref["files"].items():
        for cname, methods in f["classes"].items():
            for m, info in methods.items():
                if (cname, m) in WAIVERS:
                    continue
                checked += 1
                for side_name, side in (("js", js), ("d.ts", dts)):
                    mem = side["classes"].get(cname, {}).get("members", {}).get(m)
                    if mem is None or mem["params"] is None:
                        missing.append(f"{side_name}: {cname}.{m} missing ({rel})")
                    elif side_name == "js" and not (info["required"] <= mem["params"] == info["params"]):
                        missing.append(f"js: {cname}.{m} takes {mem['params']} parameters, the reference {info['params']} ({info['required']} required)")
                    elif side_name == "d.ts" and (mem["params"], mem["required"]) != (info["params"], info["required"]):
                        missing.append(f"d.ts: {cname}.{m} declares {mem['params']} parameters ({mem['required']} required), the reference {info['params']} ({info['required']})")
    assert not missing, "\n".join(missing)
    assert checked >= 93   # 8 classes (Viewer and Camera since round 4), 94 public methods + constructors in the fixture


def test_exported_functions_and_returned_interfaces_are_covered():
    ref, (js, dts) = _reference(), _ours()
    problems = []
    for rel, f in ref["files"].items():
        for fn, info in f["functions"].items():
            for side_name, side in (("js", js), ("d.ts", dts)):
                got = side["functions"].get(fn)
                if got is None or got["params"] != info["params"]:
                    problems.append(f"{side_name}: function {fn}: {got} vs {info}")
        for iface in ("PrefixScanner", "DynamicSortStuff"):   # what get_prefix_scanner / get_dynamic_sorter hand out: classes on this side
            for m, arity in f["interfaces"].get(iface, {}).items():
                if (iface, m) in WAIVERS:
                    continue
                for side_name, side in (("js", js), ("d.ts", dts)):
                    mem = side["classes"].get(iface, {}).get("members", {}).get(m)
                    if mem is None:
                        problems.append(f"{side_name}: {iface}.{m} missing")
                    elif arity is not None and mem["params"] is not None and not (arity <= mem["params"] <= arity + 1):   # (sort takes an optional key width)
                        problems.append(f"{side_name}: {iface}.{m} arity {mem['params']} vs {arity}")
    assert not problems, "\n".join(problems)


def test_waivers_name_things_the_reference_really_has():
    ref = _reference()
    have = set()
    for f in ref["files"].values():
        for c, ms in f["classes"].items():
            have |= {(c, m) for m in ms}
        for c, ms in f["interfaces"].items():
            have |= {(c, m) for m in ms}
    assert set(WAIVERS) <= have
    listed = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for (c, m) in WAIVERS:
        assert f"{c}.{m}" in listed, f"INTEGRATION.md does not list the waiver {c}.{m}"


def test_python_host_has_the_same_method_names():
    from webdgs_amd import ops, trainer, viewer
    ref = _reference()
    py = dict(TiledForwardPass=ops.TiledForwardPass, TiledRasterizer=ops.TiledRasterizer, TiledBackwardPass=ops.TiledBackwardPass, Optimizer=ops.Optimizer,
              DensifyPrunePass=ops.DensifyPrunePass, Trainer=trainer.Trainer, Viewer=viewer.Viewer, Camera=viewer.Camera)
    missing = []
    for f in ref["files"].values():
        for cname, methods in f["classes"].items():
            for m in methods:
                if m == "constructor" or (cname, m) in WAIVERS:
                    continue
                if not hasattr(py[cname], m):
                    missing.append(f"{cname}.{m}")
    assert not missing, missing
