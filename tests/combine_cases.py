"""The cases of the combine tests, shared by scripts/gen_combine_goldens.py (which runs the reference's own checks on
them and records what they returned or raised) and the host and GPU tests.  Everything here is data, or a function of a
case's name.

LOGIC: function name -> {case name: arguments}, JSON-able.  ``times`` entries are int64 nanoseconds (``None``: NaT);
``eds`` entries are (sonar_model, source_file, converted_raw_path)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "combine_logic.json")

_ONE_BEAM = {"Top-level": False, "Environment": False, "Platform": True, "Platform/NMEA": False, "Provenance": False,
             "Sonar": True, "Sonar/Beam_group1": True, "Vendor_specific": True}
_TWO_BEAM = {**{k: v for k, v in _ONE_BEAM.items() if k != "Vendor_specific"}, "Sonar/Beam_group2": True,
             "Vendor_specific": True}
_MODELS = ("EK60", "ES70", "AZFP", "EK80", "ES80", "EA640")


def _selection_cases():
    out = {}
    for model in _MODELS:
        ek80 = model in ("EK80", "ES80", "EA640")
        out[f"{model}/1beam/none"] = dict(sonar_model=model, has_chan_dim=_ONE_BEAM, user_channel_selection=None)
        out[f"{model}/1beam/list"] = dict(sonar_model=model, has_chan_dim=_ONE_BEAM, user_channel_selection=["a", "b"])
        out[f"{model}/1beam/dict"] = dict(sonar_model=model, has_chan_dim=_ONE_BEAM,
                                          user_channel_selection={"Sonar/Beam_group1": ["a", "b"]})
        out[f"{model}/1beam/unsorted_list"] = dict(sonar_model=model, has_chan_dim=_ONE_BEAM,
                                                   user_channel_selection=["c", "a", "b"])
        if ek80:
            out[f"{model}/2beam/none"] = dict(sonar_model=model, has_chan_dim=_TWO_BEAM, user_channel_selection=None)
            out[f"{model}/2beam/list"] = dict(sonar_model=model, has_chan_dim=_TWO_BEAM, user_channel_selection=["a", "b"])
            out[f"{model}/2beam/dict_disjoint"] = dict(
                sonar_model=model, has_chan_dim=_TWO_BEAM,
                user_channel_selection={"Sonar/Beam_group1": ["a", "b"], "Sonar/Beam_group2": ["c", "d"]})
            out[f"{model}/2beam/dict_overlap"] = dict(
                sonar_model=model, has_chan_dim=_TWO_BEAM,
                user_channel_selection={"Sonar/Beam_group1": ["a", "b"], "Sonar/Beam_group2": ["b", "c", "d"]})
            out[f"{model}/2beam/dict_one_key"] = dict(  # the second beam group has no entry: KeyError
                sonar_model=model, has_chan_dim=_TWO_BEAM, user_channel_selection={"Sonar/Beam_group1": ["b", "a"]})
    return out


_S = 1_000_000_000
_T0 = 1_700_000_000 * _S

LOGIC = {
    "_check_channel_consistency": {
        "none_pass": dict(all_chan_list=[["a", "b", "c"], ["a", "b", "c"]], ed_group="test_group", channel_selection=None),
        "none_fail": dict(all_chan_list=[["a", "b", "c"], ["a", "b"]], ed_group="test_group", channel_selection=None),
        "same_as_given": dict(all_chan_list=[["a", "b", "c"], ["a", "b", "c"]], ed_group="test_group",
                              channel_selection=["a", "b", "c"]),
        "subset": dict(all_chan_list=[["a", "b", "c"], ["a", "b", "c"]], ed_group="test_group", channel_selection=["a", "b"]),
        "subset_uneven": dict(all_chan_list=[["a", "b", "c"], ["a", "b"]], ed_group="test_group",
                              channel_selection=["a", "b"]),
        "missing_from_some": dict(all_chan_list=[["a", "c"], ["a", "b", "c"]], ed_group="test_group",
                                  channel_selection=["a", "b"]),
        "none_other_order": dict(all_chan_list=[["a", "b", "c"], ["c", "a", "b"]], ed_group="g", channel_selection=None),
        "none_same_count_other_names": dict(all_chan_list=[["a", "b"], ["a", "c"]], ed_group="g", channel_selection=None),
        "one_file": dict(all_chan_list=[["b", "a"]], ed_group="g", channel_selection=None),
        "empty_selection": dict(all_chan_list=[["a"], ["b"]], ed_group="g", channel_selection=[]),
    },
    "_create_channel_selection_dict": _selection_cases(),
    "_merge_attributes": {
        "empty_first": dict(attributes=[{"key1": ""}, {"key1": "test2"}, {"key1": "test1"}]),
        "first_wins": dict(attributes=[{"key1": "test1"}, {"key1": ""}, {"key1": "test2"}, {"key2": ""}]),
        "two_keys": dict(attributes=[{"key1": ""}, {"key2": "test1", "key1": "test2"}, {"key2": "test3"}]),
        "numbers": dict(attributes=[{"n": 0, "s": ""}, {"n": 5, "s": "x"}, {"n": 7}]),
        "all_empty": dict(attributes=[{"k": ""}, {"k": ""}]),
        "no_files": dict(attributes=[]),
        "key_order": dict(attributes=[{"b": "1"}, {"a": "2", "b": "3"}]),
    },
    "_check_ascending_ds_times": {
        "ascending": dict(dims=["channel", "ping_time"], times={"ping_time": [[_T0, _T0 + _S], [_T0 + 2 * _S], [_T0 + 3 * _S]]}),
        "equal_firsts": dict(dims=["ping_time"], times={"ping_time": [[_T0, _T0 + _S], [_T0, _T0 + 5]]}),
        "descending": dict(dims=["ping_time"], times={"ping_time": [[_T0 + 2 * _S], [_T0]]}),
        "one_second_early": dict(dims=["ping_time"], times={"ping_time": [[_T0, _T0 + 2 * _S], [_T0 + _S, _T0 + 3 * _S]]}),
        "only_firsts_count": dict(dims=["ping_time"], times={"ping_time": [[_T0, _T0 + 9 * _S], [_T0 + _S]]}),
        "first_reversed_inside": dict(dims=["ping_time"], times={"ping_time": [[_T0 + _S, _T0], [_T0 + 2 * _S]]}),
        "all_nat": dict(dims=["time1"], times={"time1": [[None], [None, None]]}),
        "some_nat": dict(dims=["time1"], times={"time1": [[None], [_T0], [_T0 - 1]]}),
        "nat_between": dict(dims=["time1"], times={"time1": [[_T0], [None], [_T0 - 1]]}),
        "two_dims_second_bad": dict(dims=["time1", "time2", "channel"],
                                    times={"time1": [[_T0], [_T0 + 1]], "time2": [[_T0 + 1], [_T0]]}),
        "no_time_dim": dict(dims=["channel", "range_sample"], times={}),
        "other_dim_ignored": dict(dims=["filenames"], times={}),
    },
    "check_eds": {
        "two_files": dict(eds=[["EK60", "/data/a.raw", None], ["EK60", "/data/b.raw", None]]),
        "converted_paths": dict(eds=[["EK80", None, "s3://bucket/x/a.zarr"], ["EK80", None, "b.nc"]]),
        "source_before_converted": dict(eds=[["EK60", "a.raw", "z.zarr"], ["EK60", "b.raw", "z.zarr"]]),
        "memory": dict(eds=[["AZFP", None, None], ["AZFP", None, None]]),
        "memory_and_file": dict(eds=[["AZFP", None, None], ["AZFP", "internal-memory", None]]),
        "file_and_memory": dict(eds=[["AZFP", "internal-memory", None], ["AZFP", None, None]]),
        "same_name_other_folder": dict(eds=[["EK60", "/x/a.raw", None], ["EK60", "/y/a.raw", None]]),
        "models_differ": dict(eds=[["EK60", "a.raw", None], ["EK80", "b.raw", None]]),
        "first_model_none": dict(eds=[[None, "a.raw", None], ["EK60", "b.raw", None]]),
        "later_model_none": dict(eds=[["EK60", "a.raw", None], [None, "b.raw", None]]),
        "one_file": dict(eds=[["EK60", "only.raw", None]]),
    },
}


def load_records():
    """The recorded answers of the reference: {function: {case: {"result": ...} | {"raised": type name}}}."""
    with open(GOLDEN) as f:
        return json.load(f)


def times_array(ticks):
    return np.array([np.iinfo(np.int64).min if t is None else t for t in ticks], dtype=np.int64).view("datetime64[ns]")


class TimesDataset:
    """What ``_check_ascending_ds_times`` reads of a dataset: ``.dims`` and ``ds[time].values``."""

    class _Var:
        def __init__(self, values):
            self.values = values

    def __init__(self, dims, times):
        self.dims = list(dims)
        self._times = times

    def __getitem__(self, name):
        return self._Var(self._times[name])


def ascending_datasets(case):
    n = max((len(v) for v in case["times"].values()), default=2)
    return [TimesDataset(case["dims"], {k: times_array(v[i]) for k, v in case["times"].items()}) for i in range(n)]


class FileStub:
    def __init__(self, sonar_model, source_file, converted_raw_path):
        self.sonar_model, self.source_file, self.converted_raw_path = sonar_model, source_file, converted_raw_path


# ---- the kernel's shapes (tests/test_gpu_combine.py) -------------------------------------------------------------------------
P_LIST = (1, 5, 70, 1, 3)
W_LIST = (1, 7, 64, 65, 257)
TYPE_PAIRS = (("int8", "int8"), ("int16", "int16"), ("int32", "int32"), ("int64", "int64"), ("float32", "float32"),
              ("float64", "float64"), ("uint8", "uint8"), ("int8", "float32"), ("int16", "float32"), ("int32", "float64"),
              ("int64", "float64"))


def fill(shape, dtype, seed):
    """Values that use every byte of the type; floats carry NaN (one with a payload), +inf and -inf."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        a = rng.standard_normal(shape).astype(dtype) * 1e3
        flat = a.reshape(-1)
        if flat.size >= 1:
            flat[::7] = np.nan
        if flat.size >= 3:
            flat[1::11] = np.inf
            flat[2::13] = -np.inf
        if flat.size >= 4:  # a NaN that is not np.nan: a bitwise copy keeps it
            flat.view(f"u{dtype.itemsize}")[3] = 0x7FA00001 if dtype.itemsize == 4 else 0x7FF4000000000001
        return a
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)


# ---- files that live on the host whatever happens (no beam group, no Environment): the logic without a GPU ---------------------
def host_file(i, chans, n_time, S, t0=_T0, model="EK60", name=None, prov=True, vendor_gain=1.0):
    """-> the keyword arguments of ``echopype_amd.EchoData``: Top-level, Platform (two time dimensions, strings, an int16
    cube with range_sample), Vendor_specific (no append dimension) and Provenance."""
    rng = np.random.default_rng(100 + i)
    C = len(chans)
    t1 = (t0 + i * 1000 * _S + np.arange(n_time) * _S).astype(np.int64).view("datetime64[ns]")
    t2 = t1[: max(1, n_time // 2)]
    order = sorted(range(C), key=lambda k: chans[k])  # per-channel values depend on the LABEL, not on the position
    rank = np.empty(C, dtype=int)
    rank[order] = np.arange(C)
    groups = {
        "Top-level": dict(coords={}, vars={}, attrs={"title": "" if i == 0 else f"survey {i}", "keywords": "EK60", "n": i}),
        "Platform": dict(
            coords={"channel": np.array(chans), "time1": t1, "time2": t2, "range_sample": np.arange(S)},
            vars={
                "latitude": (("time1",), rng.standard_normal(n_time), {"units": "degrees_north"}),
                "water_level": (("time2",), rng.standard_normal(len(t2)).astype(np.float32), {}),
                "sentence_type": (("time1",), np.array(["GGA", "RMC"] * n_time)[:n_time], {}),
                "counts": (("channel", "time1", "range_sample"),
                           (rank[:, None, None] * 1000 + rng.integers(-99, 99, (1, n_time, S))).astype(np.int16), {"long_name": "c"}),
                "wide_counts": (("time1", "range_sample"), rng.integers(-2**40, 2**40, (n_time, S)), {}),
                "transducer_offset_x": (("channel",), np.where(rank == 0, np.nan, rank * 1.5) if i == 0 else rank * 1.5, {}),
                "frequency_nominal": (("channel",), 1000.0 * (rank + 1), {}),
                "beam_type": (("channel",), (rank + 1).astype(np.int32), {}),
                "both_times": (("time1", "time2"), np.zeros((n_time, len(t2))), {}),
            },
            attrs={"platform_name": "ship", "platform_code_ICES": ""}),
        "Vendor_specific": dict(
            coords={"channel": np.array(chans), "pulse_length_bin": np.arange(3)},
            vars={"gain_correction": (("channel", "pulse_length_bin"), vendor_gain * (rank[:, None] + np.arange(3.0)), {})},
            attrs={}),
        "Sonar": dict(coords={}, vars={}, attrs={}),  # (the package's EchoData always has one)
    }
    if prov:
        groups["Provenance"] = dict(
            coords={"filenames": np.arange(1)},
            vars={"source_filenames": (("filenames",), np.array([name or f"file{i}.raw"]), {})},
            attrs={"conversion_software_name": "echopype", "conversion_software_version": "0.9", "conversion_time": f"t{i}"})
    return dict(sonar_model=model, source_file=f"/data/{name or f'file{i}.raw'}", converted_raw_path=None, groups=groups)


def as_echodata(ep, f):
    """A *file* of combine_ref -> the package's EchoData (host arrays)."""
    groups = {}
    for p, g in f["groups"].items():
        ds = ep.Dataset(coords=dict(g["coords"]), attrs=dict(g["attrs"]))
        for k, (dims, a, attrs) in g["vars"].items():
            ds[k] = (dims, np.asarray(a), dict(attrs))
        groups[p] = ds
    return ep.EchoData(f["sonar_model"], groups, source_file=f["source_file"], converted_raw_path=f.get("converted_raw_path"))
