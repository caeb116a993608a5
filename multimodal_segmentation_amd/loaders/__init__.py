"""Data containers and loaders (reference loaders/).

`data_conf` mirrors the dict of the same name in the reference's loaders/base_loader.py:5-7: data set name -> folder that holds
it.  It starts empty, so every configuration trains on the synthetic volumes; `experiment.py --data_folder PATH` (or
`conf.data_folder`) registers a folder in the format of loaders/volume_folder.py under the configured data set name, and
`loader_factory.init_loader(name)` then returns a loader that reads it.

`intensity_conf` (build-defined) sits beside it and is keyed like it: data set name -> an `intensity` block in the form of
dataset.json's that overrides the block of the folder registered under that name (or of the folder whose dataset.json carries that
name).  `experiment.py --intensity_norm ...` (or `conf.intensity`) fills it for every folder of a run; it starts empty, so each
folder is normalised as its own dataset.json says.

`bias_conf` (build-defined) does the same for the `bias_field` block (bias-field correction at load time): `experiment.py
--bias_correction ...` (or `conf.bias_field`) fills it; empty, each folder follows its own dataset.json.

`denoise_conf` (build-defined) does the same for the `denoise` block (non-local means denoising at load time): `experiment.py
--denoise ...` (or `conf.denoise`) fills it; empty, each folder follows its own dataset.json.

`align_conf` (build-defined) does the same for the `align` block (alignment of a volume's modalities by mutual information at load time):
`experiment.py --align ...` (or `conf.align`) fills it; empty, each folder follows its own dataset.json."""

data_conf = {}
intensity_conf = {}
bias_conf = {}
denoise_conf = {}
align_conf = {}
