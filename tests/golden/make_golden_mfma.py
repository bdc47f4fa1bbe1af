"""Record tests/golden/mfma_accumulate.npz on an MI355X: what v_mfma_f32_32x32x16_bf16 returns
for C + a b with one nonzero product (tools/micro/mfma_accumulate.hip, built beside its source
by the hipcc line in its header).

    python tests/golden/make_golden_mfma.py [tiles = 16] [out = tests/golden/mfma_accumulate.npz]

Also prints how many of the records tests/policy_grad_cases.py mfma_accumulate predicts."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import policy_grad_cases as pgc  # noqa: E402

TOOL = os.path.join(HERE, "..", "..", "tools", "micro", "mfma_accumulate")


def main():
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "mfma_accumulate.npz")
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "records.f32")
        print(subprocess.run([TOOL, str(tiles), raw], check=True, capture_output=True, text=True).stdout.strip())
        rec = np.fromfile(raw, dtype=np.float32).reshape(-1, 4)
    c, a, b, d = (np.ascontiguousarray(rec[:, i]) for i in range(4))
    model = pgc.mfma_accumulate(c, a, b)
    rne = (c.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    print("%d records: the model gives %d, fl32(C + a b) gives %d" % (len(c), int((model == d).sum()),
                                                                      int((rne == d).sum())))
    np.savez_compressed(out, c=c, a=a, b=b, d=d)


if __name__ == "__main__":
    main()
