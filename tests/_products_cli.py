"""Helper of tests/test_gpu_products.py (run as ONE FALNET_DETERMINISTIC=1 process: every forward of a command line then computes what it computed in
the run before): runs Test_KITTI.py's main() once per entry of the JSON file given as the second argument -- {name: [arguments]} -- with
--save-path <first argument>/<name>, and keeps what each run printed as <first argument>/<name>.stdout."""
import contextlib
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402


def main():
    out = sys.argv[1]
    for name, argv in json.load(open(sys.argv[2])).items():
        T.args = T.parser.parse_args(argv + ["--save-path", os.path.join(out, name)])
        with open(os.path.join(out, name + ".stdout"), "w") as f, contextlib.redirect_stdout(f):
            T.main()


if __name__ == "__main__":
    main()
