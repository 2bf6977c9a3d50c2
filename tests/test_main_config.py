"""Config / CLI surface of src.main (reference src/main.py:19-190) on CPU: the YAML sections resolve by name to this
package's classes, the dataset honours the sample contract of SURVEY.md 8a row A0, losses resolve torch.nn first."""
import os

import pytest
import torch
import yaml

from conftest import PKG


def _cfg():
    from src.main import Cfg
    with open(os.path.join(PKG, 'configs', 'refine_net_x4_synthetic.yaml')) as f:
        return Cfg(yaml.safe_load(f))


def test_yaml_sections_resolve_by_name():
    import src
    from src.main import _get_instance
    cfg = _cfg()
    assert cfg.main.random_seed == 'vsr' and cfg.trainer.kwargs.device == 'cuda:0'
    net = _get_instance(src.model.nets, cfg.net)
    assert type(net).__name__ == 'RefineNet' and sum(p.numel() for p in net.parameters()) == 2890993
    assert 'Trainable parameters: 2.890993 M' in repr(net)
    assert hasattr(src.runner.trainers, cfg.trainer.name) and hasattr(src.callbacks.monitor, cfg.monitor.name)
    assert hasattr(src.callbacks.loggers, cfg.logger.name) and hasattr(src.data.dataloader, cfg.dataloader.name)
    loss = _get_instance(torch.nn, cfg.losses[0])
    assert isinstance(loss, torch.nn.L1Loss)
    assert isinstance(_get_instance(src.model.metrics, cfg.metrics[0]), torch.nn.Module)


def test_dataset_sample_contract():
    import src
    from src.main import _get_instance
    cfg = _cfg()
    cfg.dataset.kwargs.update(type='train')
    ds = _get_instance(src.data.datasets, cfg.dataset)
    s = ds[3]
    F, T = 7 + 12, 7
    assert len(s['lr_imgs']) == F and len(s['hr_imgs']) == T and tuple(s['pos_code'].shape) == (F, 1)
    assert tuple(s['lr_imgs'][0].shape) == (1, 32, 32) and tuple(s['hr_imgs'][0].shape) == (1, 128, 128)
    assert float(s['pos_code'].abs().max()) <= 1.0
    loader = src.data.dataloader.Dataloader(ds, batch_size=2)
    b = next(iter(loader))
    assert len(b['lr_imgs']) == F and tuple(b['lr_imgs'][0].shape) == (2, 1, 32, 32) and tuple(b['pos_code'].shape) == (2, F, 1)
    cfg.dataset.kwargs.update(type='valid')
    dv = _get_instance(src.data.datasets, cfg.dataset)
    v = dv[0]
    assert len(v['lr_imgs']) == 30 + 12 and len(v['hr_imgs']) == 30


def test_state_dict_roundtrip_with_reference_layout(golden_dir):
    from src.model.nets import RefineNet
    c = torch.load(os.path.join(golden_dir, 'g1_tiny.pt'), weights_only=False)['x3_pos0_mem0']
    net = RefineNet(**c['kwargs'])
    net.load_state_dict(c['state_dict'])                      # a reference checkpoint loads, strict
    for k, v in net.state_dict().items():
        assert torch.equal(v, c['state_dict'][k])


REF_YAMLS = [('train', f'exp{i}_x{s}.yaml') for i, s in ((1, 4), (2, 3), (3, 2))] + \
            [('test', f'exp{i}_x{s}.yaml') for i, s in ((1, 4), (2, 3), (3, 2))]


@pytest.mark.parametrize('split,name', REF_YAMLS)
def test_reference_refinenet_yamls_resolve_unchanged(split, name, golden_dir, tmp_path):
    """The boundary claim "src.main + configs/train/refine_net/exp1_x4.yaml run unchanged" (reference src/main.py:59,
    :170-181): every section of the reference's own RefineNet YAMLs (ACDC; its *_dsb15.yaml files name a dataset class the
    reference does not contain) resolves by name against this package and constructs with the YAML's kwargs.  The YAMLs are
    read as parsed by tests/golden/make_golden.py (g8_reference_yamls.json)."""
    import json
    import src
    from src.main import Cfg, _get_instance, _losses_metrics
    with open(os.path.join(golden_dir, 'g8_reference_yamls.json')) as f:
        cfg = Cfg(json.load(f)[f'{split}/{name}'])
    # net: constructed with the YAML's kwargs, parameter count of the reference (base_net.py:11-13)
    net = _get_instance(src.model.nets, cfg.net)
    from oracle import refinenet_oracle as orc
    spec = orc.state_dict_spec(orc.Config(**cfg.net.kwargs))             # the oracle's layout is pinned to the reference (g1, g5)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(sh)) for k, sh in spec.items()]
    if cfg.net.kwargs.upscale_factor == 4:
        assert sum(p.numel() for p in net.parameters() if p.requires_grad) == 2890993
    # dataset: the class exists and takes the YAML's kwargs (synthetic cines stand in for data_dir, which does not exist here)
    cls = getattr(src.data.datasets, cfg.dataset.name)
    kw = dict(cfg.dataset.kwargs)
    kw.update(data_dir=None, pos_code_path=None, type='train' if split == 'train' else 'test')
    ds = cls(**kw)
    F = cfg.dataset.kwargs.num_frames + 2 * cfg.dataset.kwargs.num_updated_frames
    s0 = ds[0]
    if split == 'train':
        assert len(s0['lr_imgs']) == F and tuple(s0['lr_imgs'][0].shape) == (1, 32, 32)
        r = cfg.net.kwargs.upscale_factor
        assert tuple(s0['hr_imgs'][0].shape) == (1, 32 * r, 32 * r)
    # dataloader kwargs as src.main pops / updates them (main.py:46-57 of the reference)
    dk = dict(cfg.dataloader.kwargs)
    bs = dk.pop('train_batch_size', None) or dk.pop('batch_size')
    dk.pop('valid_batch_size', None)
    dk['num_workers'] = 0
    loader = getattr(src.data.dataloader, cfg.dataloader.name)(ds, batch_size=bs, **dk)
    assert loader.batch_size == bs
    loss_fns, loss_weights = _losses_metrics(cfg)
    assert [type(f).__name__ for f in loss_fns] == ['L1Loss'] and loss_weights == [1.0]
    for cm in cfg.metrics:
        assert hasattr(src.model.metrics, cm.name), cm.name
    if split == 'train':
        assert cfg.optimizer.name == 'Adam' and hasattr(torch.optim, cfg.optimizer.name)
        assert hasattr(src.callbacks.loggers, cfg.logger.name)
        mon = getattr(src.callbacks.monitor, cfg.monitor.name)(checkpoints_dir=str(tmp_path / 'checkpoints'), **cfg.monitor.kwargs)
        assert mon.early_stop == float('inf')                       # early_stop: 0 in the YAML = never
        tr = getattr(src.runner.trainers, cfg.trainer.name)
        import inspect
        assert set(cfg.trainer.kwargs) <= set(inspect.signature(tr.__init__).parameters) | \
            set(inspect.signature(src.runner.trainers.acdc_vsr_refinenet_trainer.BaseTrainer.__init__).parameters)
    else:
        pr = getattr(src.runner.predictors, cfg.predictor.name)
        import inspect
        assert set(cfg.predictor.kwargs) <= set(inspect.signature(pr.__init__).parameters) | \
            set(inspect.signature(src.runner.predictors.BasePredictor.__init__).parameters)
