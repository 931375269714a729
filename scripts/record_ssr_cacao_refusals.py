#!/usr/bin/env python
"""Writes what a front-end test module compares with (tests/test_gpu_ssr_cacao_front_ends.py, the default, or with --module tests.test_gpu_lit_front_ends the
lit draw's): every refusal text of its entry points and of their bindings, as the library and the bindings word them NOW. It is meant to be run on the state
BEFORE a change of that host code, on the GPU:

    VQHIP_LIBRARY_PATH=<libvqhip.so built from the commit before> python scripts/record_ssr_cacao_refusals.py [--module MODULE] --capi <capi.py of that commit> [--out FILE]

The module supplies make_small(), LISTENED, listen(), wrong_twice(), python_refusals() and GOLDEN, the default --out. --capi loads that file as the bindings whose
ValueErrors are recorded (it sits beside the package's abi module); without it the package's own capi.py is used."""
import argparse
import importlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--module", default="tests.test_gpu_ssr_cacao_front_ends", help="the front-end test module to record for")
    ap.add_argument("--capi", help="a capi.py to take the bindings' refusals from")
    ap.add_argument("--out", help="default: the module's GOLDEN")
    args = ap.parse_args()
    T = importlib.import_module(args.module)
    from vqengine_amd import capi
    bindings = capi
    if args.capi:
        spec = importlib.util.spec_from_file_location("vqengine_amd.capi_before", args.capi)
        bindings = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = bindings
        spec.loader.exec_module(bindings)
    out_path = args.out or T.GOLDEN
    ctx, old = capi.Context(0), bindings.Context(0)
    small = T.make_small()
    golden = {"library": {which: T.listen(ctx, small, which) for which in sorted(T.LISTENED)}, "wrong_twice": T.wrong_twice(ctx, small), "python": T.python_refusals(old, small)}
    old.close()
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out_path}: {sum(len(v) for v in golden['library'].values())} refusals of the {len(T.LISTENED)} refusal tests, {len(golden['wrong_twice'])} calls wrong twice, "
          f"{len(golden['python'])} ValueErrors; library {capi.lib_path()}")


if __name__ == "__main__":
    main()
