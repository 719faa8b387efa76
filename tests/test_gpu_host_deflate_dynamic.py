"""The host program with BVC_HOST_DEVICE_DEFLATE_CODES=1 (tuning key "bgzf_codes" on the contexts it creates; GPU): the smallest
parametrisation of tests/test_gpu_host_deflate.py run with the device deflate off, on with the fixed code and on with dynamic codes.  The
.vcf.gz walks clean as BGZF each time and inflates to the same bytes; the dynamic file is smaller than the fixed one; without
BVC_HOST_DEVICE_DEFLATE the new knob changes nothing."""
import os

import pytest

from tests import bgzf_blocks as bb
from tests.test_gpu_host import _run
from tests.test_gpu_host_deflate import _outputs, _tiles, inputs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_off_fixed_and_dynamic_inflate_to_the_same_bytes(tmp_path, inputs):  # noqa: F811
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    out = str(tmp_path / "out")
    raw, text = {}, {}
    runs = (("off", {}), ("fixed", dict(BVC_HOST_DEVICE_DEFLATE="1")), ("dynamic", dict(BVC_HOST_DEVICE_DEFLATE="1", BVC_HOST_DEVICE_DEFLATE_CODES="1")),
            ("codes alone", dict(BVC_HOST_DEVICE_DEFLATE_CODES="1")))
    for i, (name, env) in enumerate(runs):
        r = _run(exe, out, lst, fa, ["--keep_tmp"] + (["--rerun"] if i else []), dict(os.environ, BVC_HOST_PROFILE="1", **env), thread=1)
        assert r.returncode == 0, r.stderr[-2000:]
        dev, _, deflated = _tiles(r.stderr)
        assert dev > 0 and deflated == (dev if "BVC_HOST_DEVICE_DEFLATE" in env else 0), (name, r.stderr[-2000:])
        raw[name] = open(out + ".vcf.gz", "rb").read()
        bb.walk_file(raw[name])
        text[name] = _outputs(out)
        assert text[name] == text["off"], name
    print({name: len(x) for name, x in raw.items()})
    assert raw["codes alone"] == raw["off"]
    assert len(raw["dynamic"]) < len(raw["fixed"])
