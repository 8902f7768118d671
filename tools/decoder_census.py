#!/usr/bin/env python3
"""Digests and launch counts of the decoder-stack cases (tests/decoder_cases.py), one JSON object per case on stdout.

    python tools/decoder_census.py [PACKAGE_DIR] [--golden OUT.json] [--only NAME ...]

PACKAGE_DIR: the tree to import `aliparaformerasr_amd` and `oracle` from (default: this one) — a built copy of another
commit gives that commit's figures for the same cases, so two builds are compared digest by digest (bit identity of a
refactor).  Per case: SHA-256 of the raw bytes of token_ids / token_num / logits / cif_peak (and of the ids of an
ids-only run where the case asks for one; for the streaming seam: log-probs, ids, caches, with and without logits), then
the launch count of every profile class from a second, profiled run on a fresh engine.

--golden OUT.json writes the offline cases' counts as tests/golden/decoder_launch_census.json expects them: run it on the
commit BEFORE a change to the decoder walks, never on the code under test."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("package_dir", nargs="?", default=HERE)
    ap.add_argument("--golden")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(args.package_dir))
    import numpy as np
    import decoder_cases as DC
    import aliparaformerasr_amd
    print(json.dumps({"package": os.path.dirname(os.path.abspath(aliparaformerasr_amd.__file__))}), flush=True)

    golden = {}
    for case in DC.OFFLINE:
        if args.only and case.name not in args.only:
            continue
        with DC.engine(case) as eng:
            res = DC.forward(eng, case)
            dig = {"token_ids": sha(res.token_ids), "token_num": sha(res.token_num), "logits": sha(res.logits)}
            if res.cif_peak is not None:
                dig["cif_peak"] = sha(res.cif_peak)
            if case.ids_only:
                dig["token_ids_ids_only"] = sha(DC.forward(eng, case, want_logits=False).token_ids)
            DC.check_rows(case, res)
        census = DC.launch_census(case)
        golden[case.name] = census
        print(json.dumps({"case": case.name, "L": int(res.L), "digests": dig, **census}, sort_keys=True), flush=True)

    if not args.only or "O-online_decoder-m0" in args.only:
        enc, emb, lens, caches = DC.online_inputs()
        with DC.engine("O") as eng:
            logits, ids, cout = eng.online_decoder(enc, emb, lens, caches)
            _, ids2, cout2 = eng.online_decoder(enc, emb, lens, caches, want_logits=False)
        dig = {"logits": sha(logits), "ids": sha(ids), "caches": sha(np.stack(cout)),
               "ids_no_logits": sha(ids2), "caches_no_logits": sha(np.stack(cout2))}
        print(json.dumps({"case": "O-online_decoder-m0", "digests": dig}, sort_keys=True), flush=True)

    if args.golden:
        with open(args.golden, "w", encoding="utf-8") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
