"""Sample extraction, the parts that need no GPU: the fixture against the reference's own scripts, the numpy restatement of the record
layouts against the fixture, the permutation, the drivers' file discovery and the add_sequence errors."""
import os
import sys

import numpy as np
import pytest

import extract_cases as ec
from conftest import REFERENCE, ROOT

sys.path.insert(0, os.path.join(ROOT, "hevc-complexity-reduction_amd"))


@pytest.fixture(scope="module")
def golden():
    return ec.load_golden()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "Extract_Data")), reason="the reference checkout is not on this machine")
def test_fixture_is_what_the_reference_writes(golden):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_extract_golden as gen
    fresh = gen.generate(REFERENCE)
    assert sorted(fresh) == sorted(golden.files)
    for k in fresh:
        assert np.array_equal(fresh[k], golden[k]), k


@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_numpy_restatement_equals_fixture(golden, case, tmp_path):
    seqs = ec.make_inputs(case, str(tmp_path), golden["labels_" + case] if "labels_" + case in golden.files else None)
    want = golden["records_" + case]
    rb = 4992 if ec.CASES[case]["kind"] == "ai" else 16516
    assert want.size == ec.EXPECTED_COUNT[case] * rb
    assert np.array_equal(ec.np_records(case, seqs), want)


def test_real_labels_hold_more_than_a_generator_pattern(golden):
    assert set(np.unique(golden["labels_ai4"])) <= {0, 1, 2, 3} and len(np.unique(golden["labels_ai4"])) >= 3
    assert not np.array_equal(golden["labels_ai4"][:96], golden["labels_ai4"][96:192])


@pytest.mark.parametrize("count", [1, 2, 3, 22, 4096, 4097, 100003])
def test_permutation_is_a_bijection(pkg, count):
    p = pkg.ethcnn.sample_permutation(5, count)
    assert p.shape == (count,) and np.array_equal(np.sort(p), np.arange(count))
    if count >= 22:
        assert not np.array_equal(p, pkg.ethcnn.sample_permutation(6, count))
        assert not np.array_equal(p, np.arange(count))
    assert np.array_equal(p, pkg.ethcnn.sample_permutation(5, count))


def test_discovery_and_sequences_file(golden, tmp_path):
    import sequence_table as di
    seqs = ec.make_inputs("ldp", str(tmp_path / "in"))
    name, w, h, yuvs, labs = seqs[0]
    assert di.resi_file(str(tmp_path / "in"), name, 27) == yuvs[1]
    assert di.info_file(str(tmp_path / "in"), name, 37) == labs[3]
    with pytest.raises(SystemExit, match="0 files match"):
        di.info_file(str(tmp_path / "in"), name, 42)
    open(labs[3].replace("Info_2017", "Info_2018"), "wb").close()  # a second match
    with pytest.raises(SystemExit, match="2 files match"):
        di.info_file(str(tmp_path / "in"), name, 37)
    lst = tmp_path / "seqs.txt"
    lst.write_text("# my material\nSeqA_200x136 200 136\n\nSeqB_128x64 128 64  # small\n")
    assert di.parse_sequences(str(lst)) == [("SeqA_200x136", 200, 136), ("SeqB_128x64", 128, 64)]
    assert di.select(str(lst), di.INTER_INDEX, "train")[1][0] == "SeqB_128x64"
    lst.write_text("SeqA 200\n")
    with pytest.raises(SystemExit, match="name width height"):
        di.parse_sequences(str(lst))
    # the built-in table and index lists (extract_data_AI.py:19-21, extract_data_LDP_LDB_RA.py:27-29)
    assert len(di.SEQUENCES) == 212 and di.SEQUENCES[0] == ("IntraTrain_768x512", 768, 512)
    assert [len(di.INTER_INDEX[k]) for k in ("train", "valid", "test")] == [83, 10, 18]
    assert di.select(None, di.AI_INDEX, "test")[3] == ("IntraTest_4928x3264", 4928, 3264)


def test_add_sequence_errors_without_a_device(pkg, golden, tmp_path):
    E = pkg.ethcnn
    seqs = ec.make_inputs("ldp", str(tmp_path / "ldp"))
    ai = ec.make_inputs("ai1", str(tmp_path / "ai"))
    with E.SampleSet(None, "ai", [32]) as s:
        name, w, h, yuvs, labs = ai[0]
        s.add_sequence(w, h, yuvs[0], labs)
        assert s.count == 18 and s.record_bytes == 4992
        with pytest.raises(E.EthCnnError) as e:  # not a whole number of frames
            with open(yuvs[0], "ab") as f:
                f.write(b"\0" * 7)
            s.add_sequence(w, h, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(yuvs[0]) in str(e.value)
        name, w, h, yuvs, labs = ai[1]
        with open(labs[0], "r+b") as f:
            f.truncate(os.path.getsize(labs[0]) - 1)
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(labs[0]) in str(e.value)
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(60, 64, yuvs[0], labs)
        assert e.value.code == E.ERR_FORMAT
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, str(tmp_path / "missing.yuv"), labs)
        assert e.value.code == E.ERR_IO
        assert s.count == 18
        with pytest.raises(E.EthCnnError) as e:  # no context: nothing to build on
            s.build()
        assert e.value.code == E.ERR_ARG
    with E.SampleSet(None, "inter", [22, 27, 32, 37], order="ra") as s:
        name, w, h, yuvs, labs = seqs[0]
        s.add_sequence(w, h, yuvs, labs)
        assert s.count == 12 and s.record_bytes == 16516  # frame 0 skipped
        with open(yuvs[2], "ab") as f:
            f.write(b"\0" * (w * h * 3 // 2))
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs, labs)
        assert e.value.code == E.ERR_FORMAT and os.path.basename(yuvs[2]) in str(e.value)
        with pytest.raises(E.EthCnnError) as e:
            s.add_sequence(w, h, yuvs[:1], labs)
        assert e.value.code == E.ERR_ARG
    for bad in ([22, 22, 27, 32], [22, 27, 32], [22, 27, 32, 52]):
        with pytest.raises(E.EthCnnError):
            E.SampleSet(None, "inter", bad)
    with pytest.raises(E.EthCnnError):
        E.SampleSet(None, "ai", [22], order="ra")
