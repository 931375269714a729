#!/usr/bin/env python
"""Writes what tests/test_gpu_ssr_cacao_front_ends.py compares with: every refusal text of the SSR and CACAO entry points and of their bindings, as the library and
the bindings word them NOW. It is meant to be run on the state BEFORE a change of that host code, on the GPU:

    VQHIP_LIBRARY_PATH=<libvqhip.so built from the commit before> python scripts/record_ssr_cacao_refusals.py --capi <capi.py of that commit> [--out FILE]

--capi loads that file as the bindings whose ValueErrors are recorded (it sits beside the package's abi module); without it the package's own capi.py is used.
The default --out is tests/golden/ssr_cacao_refusals.json."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--capi", help="a capi.py to take the bindings' refusals from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ssr_cacao_refusals.json"))
    args = ap.parse_args()
    from tests import test_gpu_ssr_cacao_front_ends as T
    from vqengine_amd import capi
    bindings = capi
    if args.capi:
        spec = importlib.util.spec_from_file_location("vqengine_amd.capi_before", args.capi)
        bindings = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = bindings
        spec.loader.exec_module(bindings)
    ctx, old = capi.Context(0), bindings.Context(0)
    small = T.make_small()
    golden = {"library": {which: T.listen(ctx, small, which) for which in sorted(T.LISTENED)}, "wrong_twice": T.wrong_twice(ctx, small), "python": T.python_refusals(old, small)}
    old.close()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {sum(len(v) for v in golden['library'].values())} refusals of the six refusal tests, {len(golden['wrong_twice'])} calls wrong twice, "
          f"{len(golden['python'])} ValueErrors; library {capi.lib_path()}")


if __name__ == "__main__":
    main()
