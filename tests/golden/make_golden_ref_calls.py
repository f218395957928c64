#!/usr/bin/env python3
"""Writes tests/golden/ref_call_digests.json: for every test of tests/test_oracle_port_vs_ref.py and tests/test_oracle_fuzz.py,
the (name, digest) of each value the verbatim reference (oracle/_ref) handed the test, in call order.  Where oracle/_ref is not
built, those tests replay the reference's side from this file (test_oracle_port_vs_ref.pair_factory).
Needs oracle/_ref (oracle/Makefile target `ref`); a few seconds.   python tests/golden/make_golden_ref_calls.py"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "ref_call_digests.json")


def main():
    sys.path.insert(0, os.path.dirname(TESTS))
    from oracle import pyoracle
    pyoracle.build("all")
    if not pyoracle.available("ref", "array"):
        raise SystemExit("oracle/_ref is not built: the reference's sources are needed to record its calls")
    if os.path.exists(OUT):
        os.remove(OUT)
    env = dict(os.environ, FIESTA_RECORD_REF_CALLS=OUT)
    env.pop("FIESTA_REPLAY_REF_CALLS", None)
    subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                    os.path.join(TESTS, "test_oracle_port_vs_ref.py"), os.path.join(TESTS, "test_oracle_fuzz.py")],
                   env=env, check=True, cwd=os.path.dirname(TESTS))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
