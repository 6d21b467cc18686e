"""The list_occurrences.py driver (CPU, host twin): the CSV it writes for COX2, streaming above --max_rows, numbering of
the output files and the refusal of labelled queries."""
import csv
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import list_occurrences as driver  # noqa: E402
from desco_amd.data import load_data  # noqa: E402
from desco_amd.groundtruth import list_occurrences  # noqa: E402

HEXAGON = "0-1 1-2 2-3 3-4 4-5 5-0"


def read(path):
    with open(path) as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_csv_for_cox2_whole_and_streamed(tmp_path, capsys):
    with _quiet():
        graphs = load_data("COX2", root_folder=str(tmp_path / "nodata"))
        want = list_occurrences(graphs, (6, [(i, (i + 1) % 6) for i in range(6)]), backend="host")
        assert len(want) > 100
        base = ["--datasets", "COX2", "--edges", HEXAGON, "--backend", "host", "--output_dir", str(tmp_path),
                "--data_root", str(tmp_path / "nodata")]
        out = driver.main(base)
        streamed = driver.main(base + ["--max_rows", "50"])
    assert out["occurrences"].endswith("occurrences_0.csv") and streamed["occurrences"].endswith("occurrences_1.csv")
    head, rows = read(out["occurrences"])
    assert head == ["", "dataset", "graph", "v0", "v1", "v2", "v3", "v4", "v5"]
    assert len(rows) == len(want) == out["rows"]
    t = want.table()
    got = np.array([[int(x) for x in r[2:]] for r in rows])
    assert np.array_equal(got, np.stack([t[c] for c in head[2:]], axis=1))
    assert [r[0] for r in rows] == [str(i) for i in range(len(rows))] and {r[1] for r in rows} == {"COX2"}
    assert read(streamed["occurrences"]) == (head, rows)
    printed = capsys.readouterr().out
    assert f"{len(want)} occurrences in 1 chunk(s) (host)" in printed
    assert int(re.findall(r"occurrences in (\d+) chunk", printed)[1]) >= len(want) // 50       # the streamed run
    assert "25%" in printed and "wrote" in printed


class _quiet:
    """load_data warns that it uses the synthetic stand-in when the raw files are absent."""

    def __enter__(self):
        import warnings
        self._c = warnings.catch_warnings()
        self._c.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        return self._c.__exit__(*a)


def test_atlas_query_and_noninduced(tmp_path):
    with _quiet():
        out = driver.main(["--datasets", "MUTAG", "--atlas_id", "7", "--noninduced", "--backend", "host",
                           "--output_dir", str(tmp_path), "--data_root", str(tmp_path / "nodata")])
    head, rows = read(out["occurrences"])
    assert head[2:] == ["graph", "v0", "v1", "v2"]                # atlas 7 = the triangle; 6 = P3
    assert out["rows"] == len(rows)


def test_labelled_queries_are_refused_naming_the_flag(tmp_path, capsys):
    with pytest.raises(SystemExit):
        driver.main(["--edges", "0-1", "--use_node_feature", "--output_dir", str(tmp_path)])
    assert "--use_node_feature" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []
