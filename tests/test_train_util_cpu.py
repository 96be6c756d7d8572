"""Host-side rules of the --dice / --weight-map / --alpha switches and of cdnet_amd.train_util that need no GPU."""
import inspect
import types

import pytest

WMAP, CE, DICE = 1, 2, 4


def test_terms_table():
    from cdnet_amd import utils
    assert (utils.LOSS_WMAP, utils.LOSS_CE, utils.LOSS_DICE) == (WMAP, CE, DICE)
    table = {
        # (dice, weight_map, alpha): terms
        (1, 1, 0): WMAP | CE | DICE, (1, 1, 1): WMAP | CE | DICE, (1, 1, 2): WMAP | DICE,
        (0, 1, 0): WMAP | CE, (0, 1, 1): WMAP | CE, (0, 1, 2): WMAP,
        (2, 1, 0): WMAP | DICE, (2, 1, 1): WMAP | DICE, (2, 1, 2): WMAP | DICE,
        (1, 0, 0): CE | DICE, (1, 0, 1): CE | DICE, (1, 0, 2): DICE,
        (0, 0, 0): CE, (0, 0, 1): CE, (0, 0, 2): 0,
        (2, 0, 0): DICE, (2, 0, 1): DICE, (2, 0, 2): DICE,
    }
    for (dice, wm, alpha), want in table.items():
        assert utils.loss_terms(dice, wm, alpha) == want, (dice, wm, alpha)
        assert utils.loss_terms(dice, wm, float(alpha)) == want
    assert utils.loss_terms() == WMAP | CE | DICE                   # a plain Trainer's defaults


@pytest.mark.parametrize('kw', [dict(dice=3), dict(weight_map=2), dict(alpha=3), dict(alpha=0.5), dict(dice=-1)])
def test_terms_refuse_other_values(kw):
    from cdnet_amd import utils
    with pytest.raises(ValueError, match=list(kw)[0]):
        utils.loss_terms(**kw)


def test_train_util_refuses_what_is_not_built():
    from cdnet_amd import train_util
    from cdnet_amd.options import Options
    for key, sub, val in (('dice', 'model', 3), ('add_weightMap', 'model', 2), ('alpha', 'train', 3), ('multi_class', 'model', False)):
        opt = Options(isTrain=True)
        getattr(opt, sub)[key] = val
        with pytest.raises(ValueError):
            train_util._check_options(opt)
        # both entries check before they touch the loader, the model or the device
        with pytest.raises(ValueError):
            train_util.train([], None, types.SimpleNamespace(), None, 0, opt, None)
        with pytest.raises(ValueError):
            train_util.validate([], None, None, 0, opt, None)
    opt = Options(isTrain=True)
    assert train_util._check_options(opt) == (1, 1, 0.0)


def test_dam_loop_refuses_dice_other_than_1():
    from cdnet_amd import train_util_dam
    from cdnet_amd.options import Options
    model = types.SimpleNamespace(VARIANT='rev1')
    for dice in (0, 2):
        opt = Options(isTrain=True)
        opt.model['dice'] = dice
        with pytest.raises(ValueError, match='loss_direction_dice'):
            train_util_dam._check_branches(opt, model)
    for alpha, wm in ((2, 1), (0, 0), (2.0, 0)):
        opt = Options(isTrain=True)
        opt.train['alpha'], opt.model['add_weightMap'] = alpha, wm
        train_util_dam._check_branches(opt, model, alphas=(0, 1, 2))          # what train() and validate() pass
    opt.train['alpha'] = 3
    with pytest.raises(ValueError, match='alpha = 3'):
        train_util_dam._check_branches(opt, model, alphas=(0, 1, 2))


def test_signatures_are_the_references():
    from cdnet_amd import train_util
    want_train = ['train_loader', 'model', 'optimizer', 'criterion', 'epoch', 'opt', 'logger', 'get_process_worktime', 'get_process_detail',
                  'accuracy_tensor']
    want_val = ['val_loader', 'model', 'criterion', 'epoch', 'opt', 'logger', 'labeled_df_list', 'get_process_worktime', 'get_process_detail',
                'all_img_test', 'accuracy_tensor']
    for fn, want in ((train_util.train, want_train), (train_util.validate, want_val)):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps[:len(want)]] == want
        # anything beyond the reference's list (the dice out-argument) is optional
        assert all(p.default is not inspect.Parameter.empty for p in ps[len(want):])
    d = {p.name: p.default for p in inspect.signature(train_util.train).parameters.values()}
    assert (d['get_process_worktime'], d['get_process_detail'], d['accuracy_tensor']) == (1, 1, 0)
    d = {p.name: p.default for p in inspect.signature(train_util.validate).parameters.values()}
    assert (d['labeled_df_list'], d['all_img_test'], d['accuracy_tensor']) == (None, 1, 0)


def test_epoch_scores():
    from cdnet_amd import train_util
    tr = [1.5, 0.9, -1.0, 0.8, 0.31, 0.5, 0.6, 0.42]               # loss, CE, var, accu, IoU, recall, precision, F1
    va = [2.5, 0.7, 0.21, 0.4, 0.3, 0.33]                           # loss, accu, IoU, recall, precision, F1
    assert train_util.epoch_scores(tr, va) == (2.5, 0.21, 0.33)
    assert train_util.epoch_scores(tr, None) == (1.5, 0.31, 0.42)
    assert train_util.epoch_scores(tr) == (1.5, 0.31, 0.42)
    # never the constant 0 the inline loop handed to EarlyStopping and to the best-checkpoint rule
    tr2 = list(tr)
    tr2[4], tr2[7] = 0.5, 0.6
    assert train_util.epoch_scores(tr2)[1:] == (0.5, 0.6) != train_util.epoch_scores(tr)[1:]


def test_get_optimizer_checks_the_switches_before_building_a_trainer():
    from cdnet_amd import utils
    from cdnet_amd.options import Options
    for key, sub, val in (('dice', 'model', 3), ('add_weightMap', 'model', 2), ('alpha', 'train', 3)):
        opt = Options(isTrain=True)
        getattr(opt, sub)[key] = val
        with pytest.raises(ValueError):
            utils.get_optimizer(opt, None)
