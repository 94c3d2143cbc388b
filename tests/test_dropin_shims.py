"""The outer ring of the drop-in boundary on the CPU: with <repo>/dropin first on sys.path the
trainer's own import lines (main_train_restoration_with_ref_input.py:10-18) resolve to textualdegremoval_amd without a
second copy of any module, the model exposes every method the trainer calls (:177-314), EnlargedSampler reproduces
the reference's index tables (tests/golden/sampler.npz, generated from the reference), and a training script's
sequence of calls (options -> experiment folders -> dataset -> loader -> model -> step) runs on the shims up to the
first optimize_parameters, which refuses to run without a GPU (no CPU fallback on the product path)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), ROOT]), HIP_VISIBLE_DEVICES='')

IMPORT_LINES = '''
from data import create_dataloader, create_dataset
from data.data_sampler import EnlargedSampler
from data.prefetch_dataloader import CPUPrefetcher, CUDAPrefetcher
from models import create_model
from utils.logger import MessageLogger, get_root_logger, get_env_info, init_tb_logger, init_wandb_logger
from utils.utils_misc import check_resume, set_random_seed, get_time_str, make_exp_dirs, mkdir_and_rename
from utils.utils_dist import get_dist_info, init_dist
from utils.utils_options import dict2str, parse
'''


def test_trainer_import_lines_resolve_to_the_package():
    code = IMPORT_LINES + '''
import models, models.archs, data.data_sampler, utils.utils_dist
import textualdegremoval_amd.models as M, textualdegremoval_amd.models.archs as A
import textualdegremoval_amd.data.data_sampler as S, textualdegremoval_amd.utils.utils_dist as U
assert models is M and models.archs is A and data.data_sampler is S and utils.utils_dist is U
from models.archs.network_nafnet_guided_arch import NAFNetRefFusion
import textualdegremoval_amd.models.archs.network_nafnet_guided_arch as X
assert NAFNetRefFusion is X.NAFNetRefFusion
from models.image_restoration_ref_model import RefGuidedImageCleanModel as R
for m in ('resume_training', 'update_learning_rate', 'feed_train_data', 'optimize_parameters', 'get_current_learning_rate',
          'get_current_log', 'save', 'validation'):
    assert callable(getattr(R, m)), m
print('ok')
'''
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=ENV, cwd='/tmp', timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stderr[-2000:]


def test_enlarged_sampler_matches_reference_index_tables(golden_dir):
    from textualdegremoval_amd.data.data_sampler import EnlargedSampler
    g = np.load(os.path.join(golden_dir, 'sampler.npz'))
    for ci, (n, world, ratio) in enumerate(g['cases']):
        n, world = int(n), int(world)
        ratio = int(ratio) if float(ratio).is_integer() else float(ratio)
        seen = []
        for r in range(world):
            s = EnlargedSampler(list(range(n)), world, r, ratio)
            for ep in g['epochs']:
                s.set_epoch(int(ep))
                idx = list(s)
                assert len(idx) == len(s) == int(g[f'c{ci}_r{r}_e{ep}_len'])
                assert idx[:4096] == g[f'c{ci}_r{r}_e{ep}'].tolist()
            s.set_epoch(0)
            seen.append(list(s))
        # the ranks' slices interleave back into one permutation of the enlarged epoch
        total = s.total_size
        merged = [seen[i % world][i // world] for i in range(total)]
        counts = np.bincount(np.array(merged), minlength=n)
        assert counts.sum() == total and counts.max() - counts.min() <= 1


# A training script's path through the shims, written here (the reference's own trainer script is not part of this
# repository): options file -> experiment folders -> logger -> dataset / sampler / loader -> model -> first step, every
# module imported through the trainer's own import lines.  Without a GPU the step must refuse to run.
TRAIN_DRIVER = IMPORT_LINES + '''
import logging
import os
import sys
opt = parse(sys.argv[1], is_train=True)
opt['dist'] = False
opt['rank'], opt['world_size'] = get_dist_info()
make_exp_dirs(opt)
logger = get_root_logger(logger_name='basicsr', log_level=logging.INFO, log_file=os.path.join(opt['path']['log'], 'train.log'))
logger.info(dict2str(opt))
set_random_seed(opt['manual_seed'])
ds_opt = opt['datasets']['train']
train_set = create_dataset(ds_opt)
sampler = EnlargedSampler(train_set, opt['world_size'], opt['rank'], ds_opt['dataset_enlarge_ratio'])
loader = create_dataloader(train_set, ds_opt, num_gpu=opt['num_gpu'], dist=opt['dist'], sampler=sampler, seed=opt['manual_seed'])
model = create_model(opt)
batch = CPUPrefetcher(loader).next()
assert batch['lq'].shape == (2, 3, 128, 128) and batch['ref'].shape == (2, 3, 128, 128), {k: v.shape for k, v in batch.items()}
model.update_learning_rate(1, warmup_iter=opt['train'].get('warmup_iter', -1))
model.feed_train_data(batch)
model.optimize_parameters(1)
'''


def test_training_script_runs_on_the_shims_until_the_gpu_step(tmp_path):
    yml = open(os.path.join(ROOT, 'tests', 'data', 'train_nafnet_ref_synthetic_debug.yml')).read().replace('num_gpu: 1', 'num_gpu: 0')
    p = tmp_path / 'cpu.yml'
    p.write_text(yml)
    out = subprocess.run([sys.executable, '-c', TRAIN_DRIVER, str(p)], capture_output=True, text=True, cwd=str(tmp_path),
                         env=dict(ENV, TDR_EXPERIMENTS_ROOT=str(tmp_path)), timeout=300)
    log = out.stdout + out.stderr
    assert 'Dataset Dataset_SyntheticPairedWithRef - TrainSet is created.' in log, log[-3000:]
    assert 'Network: NAFNetRefFusion, with parameters: 1,409,867' in log, log[-3000:]
    assert out.returncode != 0 and 'in optimize_parameters' in log and 'NotImplementedError: HIP step needs a GPU' in log, log[-3000:]
    assert os.path.isdir(tmp_path / 'experiments' / 'debug_nafnet_ref_synthetic' / 'models')
