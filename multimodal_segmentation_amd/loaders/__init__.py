"""Data containers and loaders (reference loaders/).

`data_conf` mirrors the dict of the same name in the reference's loaders/base_loader.py:5-7: data set name -> folder that holds
it.  It starts empty, so every configuration trains on the synthetic volumes; `experiment.py --data_folder PATH` (or
`conf.data_folder`) registers a folder in the format of loaders/volume_folder.py under the configured data set name, and
`loader_factory.init_loader(name)` then returns a loader that reads it.

Beside it sits one registry (build-defined) per load-time stage of loaders/volume_folder.py (its STAGES), keyed like data_conf: data set
name -> a block in the form of dataset.json's that overrides the block of the folder registered under that name (or of the folder whose
dataset.json carries that name).  experiment.py fills them for every folder of a run from its options or the configuration; they start
empty, so each folder follows its own dataset.json.  `stage_conf` maps a stage's dataset.json key to its registry:

    intensity_conf   `intensity`    intensity normalisation                              --intensity_norm ...   / conf.intensity
    bias_conf        `bias_field`   bias-field correction                                --bias_correction ...  / conf.bias_field
    denoise_conf     `denoise`      non-local means denoising                            --denoise ...          / conf.denoise
    align_conf       `align`        alignment of a volume's modalities by mutual information  --align ...       / conf.align"""

data_conf = {}
intensity_conf = {}
bias_conf = {}
denoise_conf = {}
align_conf = {}
stage_conf = {'intensity': intensity_conf, 'bias_field': bias_conf, 'denoise': denoise_conf, 'align': align_conf}
